// nbody_f32.cpp -- host orchestration of an F = f32 handle on one shard or over index-block shards; its State holds the bodies.
//
// One handle = one reference `Simulation` object (src/shared.rs:80-97) living on one GPU.
// step_by follows brute_force.rs:84-90 / barnes_hut.rs:265-271 kernel by kernel:
//   K1 drift_half -> K4 compact (retain) -> [exchange] -> K2 | (host octree + K5) -> K3 kick_drift
// Everything is enqueued on the handle's own stream; the brute-force path never synchronises
// with the host inside nbody_steps, the Barnes-Hut path must (the octree is built on the host).
#include "nbody_engine.h"
#include "nbody_let.h"
#include "nbody_pot.h"
#include "nbody_tracer.h"
#include "nbody_external.h"
#include "nbody_mesh.h"
#include "nbody_pairs.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

namespace nbody32 {

// The bodies, their settings and the tree (EngineBodies<float>: what other units reach through bodies(h)), and what the f32 force
// passes and the step chain keep between calls.  The device and pinned blocks named here are the handle's registry's like everything else.
struct State : EngineBodies<float> {
    // symmetric all-pairs kernel (fast math; single shard: n >= Tuning::sym_min_bodies)
    nbody::SymPlan sym_plan;
    int* d_sym_bounds = nullptr;
    float4* d_planes = nullptr;
    size_t planes_cap = 0;  // float4 entries
    int sym_waves = 0;
    uint64_t sym_pairs = 0;   // unordered pairs the rotation kernel covers at the current n_local
    size_t sym_pairs_n = 0;
    // symmetric scheme across shards (kernels_bf_cross.hip)
    nbody::CrossPlan cross;
    bool cross_on = false;
    int4* d_cross_slices = nullptr;
    size_t cross_slices_cap = 0;
    float4* d_xplanes = nullptr;   // [parts.n][A][plane_stride] travelling-side sums for other shards' bodies
    float4* d_send = nullptr;      // [parts.n][plane_stride] what goes back to their owners
    size_t xplanes_cap = 0, send_cap = 0;
    int recv_plane0 = 0;           // first plane that receives the other shards' partial sums
    // the exchange of those partial sums
    bool tail_pending = false;     // the plane reduction has not been launched yet (waits for the partials)
    bool partials_in_flight = false;
    hipEvent_t ev_partials_ready = nullptr, ev_partials_done = nullptr;   // created by the first exchange
    // inside a step
    bool kick_pending = false;  // step_end asks the force pass to fuse integrate_after_force if it can
    float kick_dt = 0.f;
    bool tracer_kick = false;   // a step's tracer walk takes the kick + half drift along (dt: kick_dt)

    // Barnes-Hut with the device build, single shard: steps are enqueued without reading anything back.  A build
    // that needs the host (deeper than 21 levels, node array too small) sets a sticky flag on the device that turns
    // every later state-changing kernel into a no-op; the host looks at it at the next synchronisation point and
    // replays from the step that failed (resolve_async).
    bool async_bh = false;
    struct PendingStep { float dt; float elapsed_before; };
    std::vector<PendingStep> pending;   // steps enqueued since the host last confirmed the device's progress
    bool last_step_async = false;
    bool host_tree_once = false;        // the next force pass builds its tree on the host (the replayed step)

    // the tuning build's walks: fast walk with the most-visited records in LDS (kernels_bh.hip, variant 3)
    float4* d_walk = nullptr;    // [walk_cap + 1] records with explicit links
    int* d_unified = nullptr;    // [walk_cap + 1]
    size_t walk_cap = 0;         // nodes
    float4* d_bfs = nullptr;     // cooperative block walk (variant 5): level-order copy of the nodes
    void* d_bfs_ws = nullptr;
    size_t bfs_cap = 0;          // nodes
    float4* d_hot = nullptr;     // [hot_cap] records
    int hot_cap = 0;
    int* d_hot_info = nullptr;   // [2] slot counter, nodes flagged by the last pass
    int* h_hot_info = nullptr;   // pinned; refreshed after every walk, read after the next step's first sync
    int hot_threshold = 0;       // NodeB::hot >= this -> staged; steered so that ~hot_cap nodes qualify
    size_t hot_threshold_n = 0;  // body count the threshold was initialised for
};

namespace {

using engine::total_upper;

// the once-per-step exchange of half-drifted positions: an in-place
// all-gather of the own segment into every rank's pos_all, plus the live counts
int exchange_begin(NbodyHandle* h) {
    State& s = *h->f32;
    if (s.sh.n_seg == 1 && !h->comm_ready) return NBODY_OK;  // (a 1-rank communicator still runs the collective)
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    // comm stream: after the drift/compaction of this step, beside whatever the compute stream does next
    HIP_TRY(h, hipEventRecord(h->ev_drifted, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->comm_stream, h->ev_drifted, 0));
    TP_TRY(h, h->tp->group_begin());
    TP_TRY(h, h->tp->all_gather(s.sh.pos_all, size_t(s.sh.seg_cap) * sizeof(float4), h->comm_stream));
    TP_TRY(h, h->tp->all_gather(s.sh.seg_count, sizeof(int), h->comm_stream));
    TP_TRY(h, h->tp->group_end());
    HIP_TRY(h, hipEventRecord(h->ev_gathered, h->comm_stream));
    h->exchange_in_flight = true;
    return NBODY_OK;
}

// everything enqueued on the compute stream after this call sees the gathered positions
int exchange_wait(NbodyHandle* h) {
    if (!h->exchange_in_flight) return NBODY_OK;
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_gathered, 0));
    h->exchange_in_flight = false;
    return NBODY_OK;
}

int fail_if_hip(NbodyHandle* h, hipError_t e) { return e == hipSuccess ? NBODY_OK : fail(h, NBODY_ERR_HIP, hipGetErrorString(e)); }

// ---- Vec::push / Vec::swap_remove on a world of index-block shards (collective: every rank makes the same call).
// The global vector is the concatenation of the ranks' blocks, so push appends to the LAST rank's block and
// swap_remove(i) moves the world's last body into slot i -- across ranks if they differ (one 40-byte message).
int sharded_counts_exact(NbodyHandle* h) {   // every rank learns every block's live count
    State& s = *h->f32;
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    int rc = exchange_wait(h);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    TP_TRY(h, h->tp->all_gather(s.sh.seg_count, sizeof(int), h->stream));
    s.count_dirty = true;
    return s.sync_count(h, h->stream);
}

int sharded_add_point(NbodyHandle* h, const void* particle) {
    State& s = *h->f32;
    int rc = sharded_counts_exact(h);
    if (rc) return rc;
    const int G = s.sh.n_seg, last = G - 1;
    if (total_upper(s) >= h->cfg.capacity || s.seg_count_host[last] >= s.sh.seg_cap)
        return fail(h, NBODY_ERR_CAPACITY, "capacity exhausted (a push goes to the end of the vector: the last rank's block is full)");
    // every rank raises its bound of the last block (its grids are sized from it; the device copy arrives with the next
    // exchange); the rank that owns the block does so by storing the body
    if (s.sh.my_seg == last) return s.push_one(h, h->stream, particle);
    s.seg_count_host[last] += 1;
    return NBODY_OK;
}

int sharded_remove_point(NbodyHandle* h, size_t index) {
    State& s = *h->f32;
    int rc = sharded_counts_exact(h);
    if (rc) return rc;
    const int G = s.sh.n_seg, me = s.sh.my_seg;
    if (index >= total_upper(s)) return fail(h, NBODY_ERR_INVALID, "swap_remove index out of range");   // Vec::swap_remove panics
    int r = 0, last = G - 1;
    size_t j = index;
    while (j >= size_t(s.seg_count_host[r])) { j -= size_t(s.seg_count_host[r]); ++r; }
    while (s.seg_count_host[last] == 0) --last;
    const size_t tail = size_t(s.seg_count_host[last]) - 1;   // the world's last body: (last, tail)
    if (r == last) {
        if (me == r && j != tail) {
            HIP_TRY(h, hipMemcpyAsync(s.sh.own_pos() + j, s.sh.own_pos() + tail, sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(s.sh.vel + j, s.sh.vel + tail, sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(s.sh.acc + j, s.sh.acc + tail, sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        }
    } else if (me == last || me == r) {
        rc = s.ensure_aos(h, 2);
        if (rc) return rc;
        if (me == last) {   // the world's last body as one PointParticle record, to the rank that holds slot `index`
            nbody::launch_soa_to_aos(h->stream, s.d_aos, 10, 1, s.sh.own_pos() + tail, s.sh.vel + tail, s.sh.acc + tail);
            TP_TRY(h, h->tp->send(s.d_aos, 40, r, h->stream));
        } else {
            TP_TRY(h, h->tp->recv(s.d_aos, 40, last, h->stream));
            nbody::launch_aos_to_soa(h->stream, s.d_aos, 10, 1, s.sh.own_pos() + j, s.sh.vel + j, s.sh.acc + j);
        }
        HIP_TRY(h, hipGetLastError());
    }
    if (me == last) {
        s.n_local = tail;
        rc = s.push_own_count(h, h->stream);
        if (rc) return rc;
    } else {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    s.seg_count_host[last] -= 1;
    return comm_check(h);
}

constexpr size_t kShardedSymMinBodies = 2048; // sharded: own-own symmetric + remote one-sided from this size up

// (re)build the symmetric kernel's plan when the number of resident sets changes
int ensure_sym_plan(NbodyHandle* h) {
    State& s = *h->f32;
    const size_t set = size_t(64) * size_t(nbody::sym_bodies_per_lane(std::max<size_t>(1, s.n_local)));   // bodies of a resident set (make_sym_plan)
    const int A = int((std::max<size_t>(1, s.n_local) + set - 1) / set);  // (an empty shard still plans one set)
    const int knobs = nbody::tuning().sym_wpb * 100 + nbody::tuning().sym_rounds + nbody::tuning().sym_k * 10000 + nbody::tuning().sym_ipt * 1000000 + (nbody::tuning().sym_opp_rot ? 500000000 : 0);
    if (s.sym_plan.A == A && s.sym_plan.ipt * 64 == int(set) && s.d_sym_bounds && s.sym_waves == knobs) return NBODY_OK;
    s.sym_waves = knobs;
    s.sym_plan = nbody::make_sym_plan(int(std::max<size_t>(1, s.n_local)));
    nbody::SymPlan& p = s.sym_plan;
    s.cross_on = false;
    if (s.sh.n_seg > 1) {
        const size_t cap_pad = (size_t(s.sh.seg_cap) + 63) / 64 * 64;
        p.plane_stride = std::max(p.n_pad, cap_pad);
        if (nbody::tuning().cross_sym && s.sh.n_seg <= 2 * (nbody::CrossPartners::kMax - 1)) {
            // every unordered pair between shards once: this GPU is resident for some partners and
            // receives the partial sums the others accumulated for its bodies
            s.cross = nbody::make_cross_plan(s.sh.my_seg, s.sh.n_seg, s.sh.seg_cap, int(std::max<size_t>(1, s.n_local)));
            s.cross_on = true;
            s.recv_plane0 = p.n_planes + s.cross.k_res;
            p.n_planes += s.cross.k_res + s.cross.n_recv;
        } else {  // one-sided planes for the other shards' bodies: CU-sized 12-wave workgroups
            const int a_os = int((p.n_pad + 511) / 512);   // (k_bf_os keeps resident sets of 512 bodies whatever the symmetric kernel's are)
            p.k_os = std::max(1, std::min(256, 3072 / std::max(1, a_os)));
            p.plane_stride = std::max(p.plane_stride, size_t(a_os) * 512);   // (its padded lanes write their rows too)
            p.n_planes += p.k_os;
        }
    }
    // two cut tables of up to 127 entries: [0, 128) every set's, [128, 256) that of the sets that also meet their opposite set
    if (!s.d_sym_bounds) HIP_TRY(h, h->mem.dev(s.d_sym_bounds, 2 * 128 * sizeof(int)));
    HIP_TRY(h, hipMemcpyAsync(s.d_sym_bounds, p.bounds.data(), p.bounds.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(s.d_sym_bounds + 128, p.bounds_long.data(), p.bounds_long.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // p.bounds is pageable
    HIP_TRY(h, grow_dev(h, s.d_planes, s.planes_cap, size_t(p.n_planes) * p.plane_stride, sizeof(float4), Grow::exact));
    if (s.cross_on) {
        const nbody::CrossPlan& c = s.cross;
        if (c.slices.size() > s.cross_slices_cap)
            HIP_TRY(h, grow_dev(h, s.d_cross_slices, s.cross_slices_cap, c.slices.size() + 64, sizeof(int4), Grow::exact));
        if (!c.slices.empty()) {
            HIP_TRY(h, hipMemcpyAsync(s.d_cross_slices, c.slices.data(), c.slices.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        const size_t xneed = size_t(std::max(1, c.parts.n)) * size_t(c.A) * p.plane_stride;
        HIP_TRY(h, grow_dev(h, s.d_xplanes, s.xplanes_cap, xneed, sizeof(float4), Grow::exact));
        const size_t sneed = size_t(std::max(1, c.parts.n)) * p.plane_stride;
        HIP_TRY(h, grow_dev(h, s.d_send, s.send_cap, sneed, sizeof(float4), Grow::exact));
    }
    return NBODY_OK;
}

int bf_forces(NbodyHandle* h) {
    State& s = *h->f32;
    const float eps2 = s.g_soft * s.g_soft;  // brute_force.rs:69
    const bool fast = h->cfg.math_mode == NBODY_MATH_FAST && nbody::tuning().bf_fast_variant == 0;
    const bool sharded = s.sh.n_seg > 1;
    // Sharded: decided from the shard CAPACITY, which every rank shares.  The live counts differ from rank
    // to rank (ragged last block, bodies leaving the box), and a rank that chose another scheme than its
    // peers would neither send nor expect the partial sums the others exchange with it (a hang in RCCL).
    const bool sym = fast && (sharded ? size_t(s.sh.seg_cap) >= kShardedSymMinBodies : s.n_local >= size_t(std::max(1024, nbody::tuning().sym_min_bodies)));
    const size_t tot = total_upper(s);
    if (sym) {
        int rc = ensure_sym_plan(h);
        if (rc) return rc;
        if (s.sym_pairs_n != s.n_local) {
            s.sym_pairs = nbody::sym_main_pairs(s.sym_plan, s.n_local);
            s.sym_pairs_n = s.n_local;
        }
    }
    const nbody::SymPlan& p = s.sym_plan;
    uint64_t timed = 0;  // interactions of the launch the HIP events bracket (the dominant one)
    if (!(sym && sharded)) {
        int rc = exchange_wait(h);
        if (rc) return rc;
    }
    if (!sym) {
        ForceTimer t(h);
        if (h->cfg.math_mode == NBODY_MATH_STRICT) nbody::launch_bf_forces_strict(h->stream, s.sh, int(s.n_local), s.g, eps2);
        else nbody::launch_bf_forces_fast(h->stream, s.sh, int(s.n_local), s.g, eps2);
        timed = tot > 0 ? uint64_t(s.n_local) * uint64_t(tot - 1) : 0;
    } else if (!sharded) {
        {
            ForceTimer t(h);
            nbody::launch_bf_sym_main(h->stream, s.sh, p, s.d_sym_bounds, s.d_planes, int(s.n_local), eps2);
        }
        timed = 2 * s.sym_pairs;
        s.tail_pending = true;
    } else {
        // own shard symmetric (needs no remote data: it overlaps the exchange of positions) ...
        nbody::launch_bf_sym_main(h->stream, s.sh, p, s.d_sym_bounds, s.d_planes, int(s.n_local), eps2);
        {
            int rc = exchange_wait(h);
            if (rc) return rc;
        }
        if (s.cross_on) {
            // ... then the pairs with the partner shards, both sides; the partial sums for their bodies
            // go back to their owners before the planes are added up (forces_finish)
            const nbody::CrossPlan& c = s.cross;
            {
                ForceTimer t(h);
                nbody::launch_bf_cross(h->stream, s.sh, c, s.d_cross_slices,
                                       s.d_planes + size_t(s.recv_plane0 - c.k_res) * p.plane_stride, s.d_xplanes,
                                       s.d_send, p.plane_stride, eps2);
            }
            for (int i = 0; i < c.parts.n; ++i) {  // unordered pairs x 2, from the host's (upper-bound) counts
                const long long set = 64LL * c.ipt;
                const long long own = std::max(0LL, std::min<long long>(s.n_local, set * c.parts.a1[i]) - set * c.parts.a0[i]);
                const long long theirs = std::max(0LL, std::min<long long>(s.seg_count_host[c.parts.seg[i]], 64LL * c.parts.c1[i]) - 64LL * c.parts.c0[i]);
                timed += 2ull * uint64_t(own) * uint64_t(theirs);
            }
        } else {
            // ... then the other shards' bodies one-sided
            ForceTimer t(h);
            nbody::launch_bf_os(h->stream, s.sh, int((p.n_pad + 511) / 512), p.k_os, s.d_planes + size_t(p.n_planes - p.k_os) * p.plane_stride, p.plane_stride, eps2);
            timed = uint64_t(s.n_local) * uint64_t(tot - s.n_local);
        }
        s.tail_pending = true;
    }
    HIP_TRY(h, hipGetLastError());
    // (NbodyStats::interactions is counted on the device from the live counts: Shard::inter)
    if (tot > 0 && h->timed_this) h->stats.force_kernel_interactions += timed;
    return NBODY_OK;
}

// BarnesHutSimulation::update_forces (barnes_hut.rs:250-263): rebuild the tree from the current
// positions, then one walk per body.
int bh_walk_device_tree(NbodyHandle* h, bool* fell_back);
int bh_walk_device_tree_async(NbodyHandle* h);
int bh_walk_host_tree(NbodyHandle* h);
int step_end(NbodyHandle* h, float dt);
int step_impl(NbodyHandle* h, float dt);

// strict math with the reference leaf rule walks with the reference's nested sums (bit-exact): the store's per-lane stack, as
// many levels as the last tree is deep (the device build goes to 42; the host build reports its depth)
int setup_nested_walk(NbodyHandle* h, nbody::TreeDev* td) {
    State& s = *h->f32;
    if (h->cfg.math_mode != NBODY_MATH_STRICT || h->cfg.leaf_mode != NBODY_LEAF_REFERENCE) return NBODY_OK;
    int rc = s.tree.ensure_stack(h, s.sh.seg_cap, (s.tree.on_device ? 43 : s.tree.host.max_depth) + 2);
    if (rc) return rc;
    td->nested_stack = s.tree.d_stack;
    td->nested_stride = s.tree.stack_lanes;
    return NBODY_OK;
}

// fast math, variant 3: buffers of the LDS-staged walk and the threshold that picks the staged nodes.
// Called after this step's first host synchronisation, so h_hot_info holds the previous pass's flagged count.
int setup_lds_walk(NbodyHandle* h, nbody::TreeDev* td, size_t n_tree) {
#ifndef NBODY_TUNING
    (void)h; (void)td; (void)n_tree;   // (the experimental walks live in the tuning build)
    return NBODY_OK;
#else
    State& s = *h->f32;
    // (its stack holds the 42 levels of the device build; a deeper host-built tree is walked by k_bh_walk)
    if (h->cfg.math_mode == NBODY_MATH_FAST && nbody::tuning().bh_walk_variant == 5 && (s.tree.on_device || s.tree.host.max_depth <= 42)) {
        if (s.bfs_cap < s.tree.node_cap) {
            s.bfs_cap = 0;
            HIP_TRY(h, h->mem.dev(s.d_bfs, s.tree.node_cap * 2 * sizeof(float4)));
            HIP_TRY(h, h->mem.dev(s.d_bfs_ws, nbody::bfs_workspace_bytes(s.tree.node_cap)));
            s.bfs_cap = s.tree.node_cap;
        }
        td->bfs = s.d_bfs; td->bfs_ws = s.d_bfs_ws; td->bfs_cap = s.bfs_cap;
        return NBODY_OK;
    }
    if (h->cfg.math_mode != NBODY_MATH_FAST || nbody::tuning().bh_walk_variant != 3 || nbody::tuning().bh_hot_cap <= 0) return NBODY_OK;
    const int M = std::min(nbody::tuning().bh_hot_cap, 5000);  // 160 KB of LDS per CU, 32 B per record
    if (s.walk_cap < s.tree.node_cap) {
        s.walk_cap = 0;
        HIP_TRY(h, h->mem.dev(s.d_walk, (s.tree.node_cap + 1) * 2 * sizeof(float4)));
        HIP_TRY(h, h->mem.dev(s.d_unified, (s.tree.node_cap + 1) * sizeof(int)));
        s.walk_cap = s.tree.node_cap;
    }
    if (s.hot_cap != M) {
        s.hot_cap = 0;
        HIP_TRY(h, h->mem.dev(s.d_hot, size_t(M) * 2 * sizeof(float4)));
        HIP_TRY(h, hipMemsetAsync(s.d_hot, 0, size_t(M) * 2 * sizeof(float4), h->stream));
        s.hot_cap = M;
        s.hot_threshold_n = 0;
    }
    if (!s.d_hot_info) {
        HIP_TRY(h, h->mem.dev(s.d_hot_info, 2 * sizeof(int)));
        HIP_TRY(h, hipMemsetAsync(s.d_hot_info, 0, 2 * sizeof(int), h->stream));
        HIP_TRY(h, h->mem.pin(s.h_hot_info, 2 * sizeof(int)));
        s.h_hot_info[0] = s.h_hot_info[1] = 0;
    }
    if (s.hot_threshold_n == 0 || n_tree > 2 * s.hot_threshold_n || 2 * n_tree < s.hot_threshold_n) {
        // first guess: the grandparent holds 1/64 of the bodies (2 500 nodes at N = 65 536 Plummer)
        s.hot_threshold = int(std::max<size_t>(8, n_tree / 64));
        s.hot_threshold_n = std::max<size_t>(1, n_tree);
    } else {
        const int flagged = s.h_hot_info[1];
        if (flagged > M) s.hot_threshold = s.hot_threshold + s.hot_threshold / 8 + 1;
        else if (flagged < M - M / 3 && s.hot_threshold > 2) s.hot_threshold = s.hot_threshold - s.hot_threshold / 8 - 1;
    }
    td->walk = s.d_walk; td->unified = s.d_unified; td->hot = s.d_hot; td->hot_info = s.d_hot_info;
    td->hot_cap = M; td->hot_threshold = s.hot_threshold;
    return NBODY_OK;
#endif
}

// the cells' tensors from the node array as it now stands on the device (k_tree_quad), for the walk that follows
// (sized like the node array: a step without read-back knows its capacity only, and the build's node count on the device)
int fill_quadrupoles(NbodyHandle* h, const nbody::TreeDev& td, bool any_nodes) {
    State& s = *h->f32;
    HIP_TRY(h, grow_dev(h, h->d_quad, h->quad_cap, s.tree.node_cap, nbody::kQuadRecBytes, Grow::quarter));
    const bool counted_on_device = td.n_order_dev != nullptr;
    if (any_nodes) nbody::launch_tree_quad(h->stream, td.nodes, td.n_nodes, h->d_quad, counted_on_device ? s.tree.bufs.d_info : nullptr, td.poison);
    return NBODY_OK;
}

// the tracers' walk of the tree the body pass has just built, with the kick + half drift when a step asked for them
int tracer_tree_forces(NbodyHandle* h, const nbody::TreeDev& td) {
    State& s = *h->f32;
    const bool kick = s.tracer_kick;
    s.tracer_kick = false;
    return nbody::tracer::tree_forces(h, td, kick ? &s.kick_dt : nullptr);
}

// the end of every f32 force pass: the buffers of the strict and the experimental walks, the walk over td (+ the kick and half
// drift when a step asked for them and the plane reduction can take them along)
int walk_tree(NbodyHandle* h, nbody::TreeDev& td, size_t n_tree) {
    State& s = *h->f32;
    if (h->pot.walking) {   // a tree call: NBODY_POTENTIAL_TREE_QUADRUPOLE wants the tensors of the tree just built (quad_call: nbody_tree_export_quadrupoles)
        h->quad_call = h->pot.quad;
        if (h->pot.quad) {
            int rc = fill_quadrupoles(h, td, td.n_nodes > 0);
            if (rc) return rc;
        }
    }
    if (h->pot.walking == kWalkField) {   // nbody_field_at(NBODY_POTENTIAL_TREE): the caller walks this tree for its probes, batch by batch
        FieldBufs& f = h->field;
        f.nodes = td.nodes; f.n_nodes = td.n_nodes; f.K = td.n_split;
        f.first = td.split_first; f.anc = td.split_anc; f.n_anc = td.split_n_anc;
        f.quad = h->pot.quad ? h->d_quad : nullptr;
        HIP_TRY(h, hipGetLastError());
        return NBODY_OK;
    }
    if (h->pot.walking) {   // nbody_potentials(NBODY_POTENTIAL_TREE): the same tree, order and split points, walked for potentials
        const size_t stride = (size_t(std::max(td.n_order, 1)) + 63) / 64 * 64;
        int rc = nbody::pot::ensure_planes(h, size_t(td.n_split) * stride);
        if (rc) return rc;
        if (h->pot.quad)
            nbody::launch_bh_pot_walk_quad(h->stream, s.sh.own_pos(), td, h->d_quad, s.g_soft * s.g_soft, s.theta2, h->pot.d_planes, stride,
                                           h->pot.d_sum, h->pot.d_counts);
        else
            nbody::launch_bh_pot_walk(h->stream, s.sh.own_pos(), td, s.g_soft * s.g_soft, s.theta2, h->pot.d_planes, stride, h->pot.d_sum,
                                      h->pot.d_counts);
        HIP_TRY(h, hipGetLastError());
        return NBODY_OK;
    }
    h->quad_pass = h->multipole == NBODY_MULTIPOLE_QUADRUPOLE;
    h->quad_call = false;
    if (h->quad_pass) {   // nbody_set_multipole(h, 2): the cells' tensors from the node array as it now stands on the device, then the walk that uses them
        int rc = fill_quadrupoles(h, td, td.n_order > 0);
        if (rc) return rc;
        ForceTimer t(h);
        int kicked = 0;
        nbody::launch_bh_walk_quad(h->stream, s.sh, td, h->d_quad, s.g, s.g_soft * s.g_soft, s.theta2, h->d_counters,
                                   h->cfg.leaf_mode == NBODY_LEAF_DIRECT, s.kick_pending ? &s.kick_dt : nullptr, &kicked);
        if (kicked) s.kick_pending = false;
        HIP_TRY(h, hipGetLastError());
        return tracer_tree_forces(h, td);   // (tracers walk monopoles whatever the multipole setting)
    }
    int rc = setup_nested_walk(h, &td);
    if (!rc) rc = setup_lds_walk(h, &td, n_tree);
    if (rc) return rc;
    {
        ForceTimer t(h);
        int kicked = 0;
        nbody::launch_bh_walk(h->stream, s.sh, td, s.g, s.g_soft * s.g_soft, s.theta2,
                              h->cfg.math_mode == NBODY_MATH_FAST, h->d_counters, h->cfg.leaf_mode == NBODY_LEAF_DIRECT,
                              s.kick_pending ? &s.kick_dt : nullptr, &kicked);
        if (kicked) s.kick_pending = false;  // the plane reduction applied the kick + half drift
    }
    if (td.hot_cap > 0) HIP_TRY(h, hipMemcpyAsync(s.h_hot_info, s.d_hot_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipGetLastError());
    return tracer_tree_forces(h, td);   // the tracers' walk of the same tree, before anything overwrites it
}

// segments of the walk over the tree just built (a field call walks its probes, not the bodies)
int split_segments(const NbodyHandle* h, const TreeBuilt& t) {
    State& s = *h->f32;
    if (h->pot.walking == kWalkField) return field_split_plan(h->field.n_points, size_t(t.n_nodes));
    return walk_split_plan(t.n_order, h->cfg.math_mode != NBODY_MATH_STRICT || h->pot.walking, s.theta2, size_t(t.n_nodes)).segments;
}
// the walk over it, once the split points of its K segments are listed
int walk_built(NbodyHandle* h, const TreeBuilt& t, int K) {
    State& s = *h->f32;
    nbody::TreeDev td;
    td.nodes = s.tree.d_nodes; td.n_nodes = t.n_nodes;
    td.order = t.order; td.n_order = int(t.n_order);
    walk_split_view(s.tree.split, K, size_t(s.sh.seg_cap), &td);
    return walk_tree(h, td, t.n_tree);
}

int bh_forces(NbodyHandle* h) {
    State& s = *h->f32;
    {
        int rc = exchange_wait(h);
        if (rc) return rc;
    }
    s.last_step_async = false;
    if (h->cfg.tree_build == NBODY_TREE_DEVICE && !s.host_tree_once) {
        // no read-back at all: single shard, the plain or the strict walk (the experimental walks want the node count)
        const bool plain_walk = h->cfg.math_mode == NBODY_MATH_STRICT || nbody::tuning().bh_walk_variant == 0;
        if (s.async_bh && (plain_walk || h->multipole == NBODY_MULTIPOLE_QUADRUPOLE) && !nbody::tuning().bh_walk_debug) return bh_walk_device_tree_async(h);
        int rc = resolve_async(h);
        if (rc) return rc;
        bool fell_back = false;
        rc = bh_walk_device_tree(h, &fell_back);
        if (rc || !fell_back) return rc;
        // deeper than 42 levels somewhere: this step's tree comes from the host build below
    }
    s.host_tree_once = false;
    return bh_walk_host_tree(h);
}

// the force pass on the tree built on the host
int bh_walk_host_tree(NbodyHandle* h) {
    State& s = *h->f32;
    Shard& sh = s.sh;
    TreeBuilt t;
    int rc = s.tree.build_on_host(h, s, &t);
    if (rc) return rc;
    // split the node range over several waves per body group when there are too few bodies to fill the chip (>= 8 waves per
    // SIMD wanted: the walk is bound by the latency of dependent loads).  ~3 waves per wave slot of the chip (256 CUs x 32),
    // handed out heaviest first (nbody::tuning().bh_walk_order): the launch lasts as long as its slowest wave, and smaller
    // pieces started in the right order shorten that tail (N = 65 536: 24 segments 0.310 ms, 8 segments 0.336 ms; tools/tune_bh_order.py)
    const int K = split_segments(h, t);
    rc = s.tree.split.ensure(h, K, size_t(sh.seg_cap));
    if (!rc) rc = s.tree.split.list_on_host(h, h->stream, s.tree.host.nodes, t.n_nodes, K);
    if (rc) return rc;
    return walk_built(h, t, K);
}

// Barnes-Hut force pass with the octree built on the device (kernels_tree.hip): no positions go to
// the host, no node array comes back; one 8-byte read-back (node count, flags) per step.
int bh_walk_device_tree(NbodyHandle* h, bool* fell_back) {
    State& s = *h->f32;
    TreeBuilt t;
    int rc = s.tree.build_on_device(h, s, nbody::tuning().bh_walk_variant == 3, nullptr, &t);
    *fell_back = t.fell_back;
    if (rc || t.fell_back) return rc;
    const int K = split_segments(h, t);
    rc = s.tree.split.ensure(h, K, size_t(s.sh.seg_cap));
    if (rc) return rc;
    if (t.n_tree > 0) s.tree.split.list_on_device(h->stream, s.tree.work, int(t.n_tree), t.n_nodes, K);
    return walk_built(h, t, K);
}

// The same force pass with nothing read back: the node count, the live body count and the build's flags stay on the
// device (TreeBuildBufs::d_info); the split points are placed by k_tree_split_anc from the device's node count, the walk takes
// its body count from the device, and a build that needs the host poisons the run (see State::async_bh).
int bh_walk_device_tree_async(NbodyHandle* h) {
    State& s = *h->f32;
    Shard& sh = s.sh;
    auto t1 = clk::now();
    TreeBuildBufs& tb = s.tree.bufs;
    int rc = tb.ensure(h, size_t(sh.seg_cap), 0);
    if (rc) return rc;
    const size_t n_upper = s.n_local;   // an upper bound of the live count
    rc = s.tree.ensure_dev(h, TreeTypes<float>::kNodesPerBody * n_upper + 64, n_upper);
    if (rc) return rc;
    if (s.pending.empty()) HIP_TRY(h, hipMemsetAsync(h->d_poison + 1, 0, sizeof(int), h->stream));   // steps completed: counted from here
    // (a tree has at least as many nodes as bodies)
    const int K = walk_split_plan(n_upper, h->cfg.math_mode != NBODY_MATH_STRICT, s.theta2, n_upper).segments;
    rc = s.tree.split.ensure(h, K, size_t(sh.seg_cap));
    if (rc) return rc;
    // the walk's split points ride in the build's last launch (they also make a build that needs the host sticky: Shard::poison)
    const nbody::TreeSplitReq req = s.tree.split.request(K, tb.d_info, h->d_poison);
    nbody::TreeDevWork& work = s.tree.work;
    if (nbody::build_octree_device(h->stream, sh.own_pos(), sh.own_count(), int(n_upper), s.center, s.width, tb.ws, size_t(sh.seg_cap),
                                   s.tree.d_nodes, int(s.tree.node_cap), s.tree.d_order, tb.d_info, &work, 0, n_upper > 0 ? &req : nullptr) != 0)
        return fail(h, NBODY_ERR_HIP, "device octree build: rocPRIM call failed");
    HIP_TRY(h, hipGetLastError());
    h->stats.tree_build_ms += ms_since(t1);   // (enqueue time: nothing is waited for)
    s.tree.on_device = true;
    if (n_upper == 0)   // (no build was enqueued: the empty root's one segment, as a launch of its own)
        s.tree.split.list_on_device(h->stream, work, 0, int(s.tree.node_cap), K, tb.d_info, h->d_poison);
    nbody::TreeDev td;
    td.nodes = s.tree.d_nodes; td.n_nodes = int(s.tree.node_cap);   // (the plain walks end at the split points, not at n_nodes)
    td.order = s.tree.d_order; td.n_order = int(n_upper);
    td.n_order_dev = tb.d_info + 2;
    td.poison = h->d_poison;
    walk_split_view(s.tree.split, K, size_t(sh.seg_cap), &td);
    rc = walk_tree(h, td, n_upper);
    if (rc) return rc;
    s.last_step_async = true;
    s.count_dirty = true;
    return NBODY_OK;
}

// ---- the partial sums other GPUs accumulated for the own bodies (symmetric scheme across shards)
int partials_begin(NbodyHandle* h) {
    State& s = *h->f32;
    if (!(s.cross_on && s.tail_pending) || s.cross.parts.n + s.cross.n_recv == 0) return NBODY_OK;
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    const nbody::CrossPlan& c = s.cross;
    const size_t S = s.sym_plan.plane_stride;
    const size_t bytes = size_t(s.sh.seg_cap) * sizeof(float4);
    if (!s.ev_partials_ready) {
        HIP_TRY(h, hipEventCreateWithFlags(&s.ev_partials_ready, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&s.ev_partials_done, hipEventDisableTiming));
    }
    HIP_TRY(h, hipEventRecord(s.ev_partials_ready, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->comm_stream, s.ev_partials_ready, 0));
    TP_TRY(h, h->tp->group_begin());
    for (int i = 0; i < c.parts.n; ++i)
        TP_TRY(h, h->tp->send(s.d_send + size_t(i) * S, bytes, c.parts.seg[i], h->comm_stream));
    for (int i = 0; i < c.n_recv; ++i)
        TP_TRY(h, h->tp->recv(s.d_planes + size_t(s.recv_plane0 + i) * S, bytes, c.recv_from[i], h->comm_stream));
    TP_TRY(h, h->tp->group_end());
    HIP_TRY(h, hipEventRecord(s.ev_partials_done, h->comm_stream));
    s.partials_in_flight = true;
    return NBODY_OK;
}

int partials_wait(NbodyHandle* h) {
    State& s = *h->f32;
    if (!s.partials_in_flight) return NBODY_OK;
    HIP_TRY(h, hipStreamWaitEvent(h->stream, s.ev_partials_done, 0));
    s.partials_in_flight = false;
    return NBODY_OK;
}

// mesh gravity: the pass is the mesh field for bodies and tracers, with the step's kicks when it asked for them (as the fused
// tail takes them); no pair kernel runs
int mesh_forces(NbodyHandle* h) {
    State& s = *h->f32;
    int rc = exchange_wait(h);
    if (rc) return rc;
    rc = nbody::mesh::pass<float>(h, s.sh, s.n_local, double(s.g), s.kick_pending ? &s.kick_dt : nullptr, s.tracer_kick ? &s.kick_dt : nullptr);
    if (!rc) s.kick_pending = false;
    return rc;
}

// everything of the force pass that needs no other GPU's partial sums
int forces_begin(NbodyHandle* h) {
    if (nbody::mesh::on(h)) return mesh_forces(h);
    return h->cfg.method == NBODY_BARNES_HUT ? bh_forces(h) : bf_forces(h);
}

// the plane reduction (with the kick + half drift when a step asked for it)
int forces_finish(NbodyHandle* h) {
    State& s = *h->f32;
    if (!s.tail_pending) return NBODY_OK;
    s.tail_pending = false;
    const float eps2 = s.g_soft * s.g_soft;
    nbody::launch_bf_sym_tail(h->stream, s.sh, s.sym_plan, s.d_planes, int(s.n_local), s.g, eps2,
                              s.kick_pending ? &s.kick_dt : nullptr);
    s.kick_pending = false;
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

int forces(NbodyHandle* h) {
    int rc = forces_begin(h);
    if (rc) return rc;
    rc = partials_begin(h);
    if (rc) return rc;
    rc = partials_wait(h);
    if (rc) return rc;
    return forces_finish(h);
}

int step_end(NbodyHandle* h, float dt) {
    int rc = step_forces(h, dt);
    if (rc) return rc;
    rc = partials_begin(h);
    if (rc) return rc;
    rc = partials_wait(h);
    if (rc) return rc;
    return step_finish(h, dt);
}

int step_impl(NbodyHandle* h, float dt) {
    State& s = *h->f32;
    const float elapsed_before = s.elapsed;
    int rc = step_begin(h, dt);
    if (rc) return rc;
    rc = exchange_begin(h);   // the force pass waits for it where it first needs remote bodies
    if (rc) return rc;
    rc = step_end(h, dt);
    if (rc) return rc;
    if (s.last_step_async) {   // nothing was read back: remember the step until the device's progress is confirmed
        s.pending.push_back(State::PendingStep{dt, elapsed_before});
        if (s.pending.size() >= 4096) rc = resolve_async(h);
    }
    return rc;
}

// NBODY_POTENTIAL_TREE on a spatial rank.  After a step the bodies have half-drifted and some lie outside their rank's key
// range; the slice-and-halo build needs every rank's bodies to BE a key range, so the pass has to migrate them -- and the call
// must migrate nothing, redraw no bound and touch no balance state.  So the pass runs on a scratch clone of the rank
// (nbody_clone: bodies, ids, visit-count weights, bounds) that borrows this handle's transport for its exchanges and is
// destroyed afterwards: in the clones' world the strays migrate, every rank builds its slice, receives its halo and walks the
// nodes it holds for potentials (let::potential_pass: the force pass, last phase swapped).  The sums then go home: every rank
// all-gathers {index in the uploaded vector, S} of the bodies it walked, and each owner picks out its own bodies by index.
// The handle itself is read, never written: bodies, bounds, weights, prediction, statistics and the host's view of the count
// stay as they were.  counts = what the clone of this rank walked.
int spatial_walk(NbodyHandle* h, NbodyHandle* twin, int n_orig) {
    State& s = *h->f32;
    const int G = h->cfg.world_size, cap = s.sh.seg_cap;
    PotBufs& p = h->pot;
    int rc = nbody::let::potential_pass(twin);
    if (rc) return fail(h, rc, twin->err);
    rc = nbody::pot::begin(h, size_t(cap));
    if (rc) return rc;
    HIP_TRY(h, grow_dev(h, p.d_rec, p.rec_cap, size_t(G) * size_t(cap), sizeof(nbody::PotRec), Grow::quarter));
    const size_t n_ids = size_t(h->cfg.capacity) + 1;
    HIP_TRY(h, grow_dev(h, p.d_slot_of, p.slot_cap, n_ids, sizeof(int), Grow::quarter));
    if (!p.d_rec_count) HIP_TRY(h, h->mem.dev(p.d_rec_count, sizeof(int) * size_t(G)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the counters' reset: what follows is ordered on the clone's stream)
    hipStream_t ts = twin->stream;
    nbody::PotRec* rec = static_cast<nbody::PotRec*>(p.d_rec);
    const Shard& tsh = twin->f32->sh;
    nbody::launch_pot_pack(ts, tsh.ids, twin->pot.d_sum, tsh.own_count(), cap, rec + size_t(h->cfg.rank) * size_t(cap));
    HIP_TRY(h, hipMemcpyAsync(p.d_rec_count + h->cfg.rank, tsh.own_count(), sizeof(int), hipMemcpyDeviceToDevice, ts));
    if (twin->comm_ready) {
        TP_TRY(twin, twin->tp->group_begin());
        TP_TRY(twin, twin->tp->all_gather(rec, size_t(cap) * sizeof(nbody::PotRec), ts));
        TP_TRY(twin, twin->tp->all_gather(p.d_rec_count, sizeof(int), ts));
        TP_TRY(twin, twin->tp->group_end());
    }
    HIP_TRY(h, hipMemsetAsync(p.d_slot_of, 0xFF, n_ids * sizeof(int), ts));
    nbody::launch_pot_scatter(ts, s.sh.ids, s.sh.own_count(), n_orig, p.d_slot_of, int(std::min<size_t>(n_ids, 0x7fffffff)), rec, p.d_rec_count, G, cap, p.d_sum);
    HIP_TRY(h, hipMemcpyAsync(p.d_counts, twin->pot.d_counts, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ts));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(ts));
    if (twin->tp) { rc = twin->tp->check(); if (rc) return fail(h, rc, twin->tp->error()); }
    return NBODY_OK;
}

int spatial_potentials(NbodyHandle* h, size_t* n_own, nbody::PotBodies* bodies, double* g) {
    State& s = *h->f32;
    if (!s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    if (h->cfg.world_size > 1 && !h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    NbodyHandle* twin = nullptr;
    int rc = NBODY_OK, n_orig = 0;
    {   // (nbody_clone refreshes the host's view of the count; the next walk's shape is drawn from the bound)
        engine::PotView<float> view(s);
        rc = nbody_clone(h, &twin);
        n_orig = int(s.n_local);   // exact now
    }
    if (rc) return fail(h, rc, std::string("nbody_potentials: scratch clone: ") + nbody_last_error(nullptr));
    twin->tp = std::move(h->tp);          // the clones' world talks over this world's transport
    twin->comm_ready = h->comm_ready;
    nbody::bind_tuning(&twin->tune);
    rc = spatial_walk(h, twin, n_orig);
    if (rc && !twin->err.empty()) h->err = twin->err;
    h->tp = std::move(twin->tp);
    twin->comm_ready = false;
    nbody::bind_tuning(&h->tune);
    nbody_destroy(twin);
    (void)hipSetDevice(h->device);
    if (rc) return rc;
    bodies->pos_all = s.sh.pos_all; bodies->vel = s.sh.vel; bodies->seg_count = s.sh.seg_count;
    bodies->f64 = 0; bodies->n_seg = 1; bodies->seg_cap = s.sh.seg_cap; bodies->my_seg = 0;
    bodies->world = h->comm_ready ? h->cfg.world_size : 1;
    *g = double(s.g);
    *n_own = size_t(n_orig);
    return NBODY_OK;
}

}  // namespace

EngineBodies<float>& bodies(NbodyHandle* h) { return *h->f32; }
const EngineBodies<float>& bodies(const NbodyHandle* h) { return *h->f32; }

int create(NbodyHandle* h) {
    State* sp = new State();
    h->f32 = sp;
    State& s = *sp;
    Shard& sh = s.sh;
    int rc = s.alloc(h, h->stream, h->shape);
    if (rc) return rc;
    HIP_TRY(h, h->mem.dev(h->d_poison, 2 * sizeof(int)));
    HIP_TRY(h, hipMemsetAsync(h->d_poison, 0, 2 * sizeof(int), h->stream));
    if (h->cfg.method == NBODY_BARNES_HUT) {
        rc = s.tree.alloc_host(h, sh);
        if (rc) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const char* v = std::getenv("NBODY_BH_ASYNC");
    sp->async_bh = h->cfg.method == NBODY_BARNES_HUT && h->cfg.tree_build == NBODY_TREE_DEVICE && h->cfg.world_size == 1 &&
                   h->cfg.shard_mode != NBODY_SHARD_SPATIAL && !(v && v[0] == '0');
    if (sp->async_bh) sh.poison = h->d_poison;
    return NBODY_OK;
}

void destroy(NbodyHandle* h) {
    State* s = h->f32;
    if (!s) return;
    if (s->ev_partials_ready) (void)hipEventDestroy(s->ev_partials_ready);
    if (s->ev_partials_done) (void)hipEventDestroy(s->ev_partials_done);
    delete s;   // (its device and pinned blocks are the handle's registry's)
    h->f32 = nullptr;
}

int clone_state(NbodyHandle* src, NbodyHandle* dst) {
    int rc = src->f32->sync_count(src, src->stream);
    if (rc) return fail(dst, rc, src->err);
    rc = fail_if_hip(dst, hipStreamSynchronize(src->stream));
    if (!rc) rc = dst->f32->copy_from(dst, dst->stream, *src->f32);
    if (!rc) rc = fail_if_hip(dst, hipStreamSynchronize(dst->stream));
    if (rc) return fail(dst, rc, "clone copy: " + dst->err);
    dst->multipole = src->multipole;
    dst->search.mode = src->search.mode;   // (the clone's statistics start at zero)
    dst->first_global = src->first_global; dst->n_at_upload = src->n_at_upload;
    // like the reference's BH clone (barnes_hut.rs:113-135) the tree is not carried over; neither
    // are the communicator (call nbody_comm_init on the clone) and the statistics
    return NBODY_OK;
}

int upload(NbodyHandle* h, const void* aos, size_t n, size_t stride) {
    const int rc = resolve_async(h);
    return rc ? rc : engine::upload(h, *h->f32, aos, n, stride);
}

int download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out) {
    State& s = *h->f32;
    int rc = resolve_async(h);
    if (rc) return rc;
    return s.download_own(h, h->stream, aos, cap, stride, n_out, comm_check);   // (bodies of a run whose exchange broke down are not handed out as results)
}

int count(NbodyHandle* h, size_t* n_out) {
    const int rc = resolve_async(h);
    return rc ? rc : engine::count(h, *h->f32, n_out);
}

int count_global(NbodyHandle* h, size_t* n_out) {
    const int rc = resolve_async(h);
    return rc ? rc : engine::count_global(h, *h->f32, n_out);
}

int add_point(NbodyHandle* h, const void* particle) {
    State& s = *h->f32;
    if (s.sh.n_seg != 1) return sharded_add_point(h, particle);
    int rc = resolve_async(h);
    if (rc) return rc;
    return s.push_one(h, h->stream, particle);
}

int remove_point(NbodyHandle* h, size_t index) {
    State& s = *h->f32;
    if (s.sh.n_seg != 1) return sharded_remove_point(h, index);
    int rc = resolve_async(h);
    if (rc) return rc;
    return s.swap_remove_one(h, h->stream, index);
}

int merge_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts) {
    // (an f32 handle keeps nothing beside the count that a removal makes stale: every force pass builds its tree anew)
    return nbody::pairs::merge_contacts<float>(h, *h->f32, radius, list, cap, n_contacts, nullptr,
                                               [](NbodyHandle* hh, int n_upper) { nbody::launch_compact(hh->stream, hh->f32->sh, n_upper); });
}

int init(NbodyHandle* h) {
    h->f32->elapsed = 0.f;  // brute_force.rs:49; the reference's BH init also builds a tree that the
                            // first update_forces rebuilds before any use (barnes_hut.rs:232-235, 251-254)
    return NBODY_OK;
}

// Where did the device get to?  Confirms the steps enqueued without read-back; if a build poisoned the run, finishes
// the failed step with the host build (which handles any depth) and enqueues the rest again.
int resolve_async(NbodyHandle* h) {
    if (!h->f32 || !h->f32->async_bh) return NBODY_OK;
    State& s = *h->f32;
    for (int round = 0; round < 1000000; ++round) {
        HIP_TRY(h, hipMemcpyAsync(h->h_poison, h->d_poison, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (s.tree.bufs.d_info) HIP_TRY(h, hipMemcpyAsync(h->h_poison + 2, s.tree.bufs.d_info, 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const int flags = h->h_poison[0], done = h->h_poison[1];
        if (!flags) {
            if (s.tree.on_device && s.tree.bufs.d_info) {   // what the last build produced
                s.tree.n_nodes = size_t(h->h_poison[2]);
                h->stats.tree_nodes = uint64_t(h->h_poison[2]);
            }
            s.pending.clear();
            return NBODY_OK;
        }
        // poisoned: steps [0, done) are complete, step `done` has drifted and compacted, nothing after it has run
        std::vector<State::PendingStep> rest;
        if (size_t(done) < s.pending.size()) rest.assign(s.pending.begin() + done, s.pending.end());
        s.pending.clear();
        HIP_TRY(h, hipMemsetAsync(h->d_poison, 0, 2 * sizeof(int), h->stream));
        if (flags & 2) {   // more nodes than the array holds: double it (the bound 4 n + 64 did not hold for this set)
            int rc = s.tree.ensure_dev(h, 2 * s.tree.node_cap + 64, s.n_local);
            if (rc) return rc;
        }
        if (rest.empty()) {   // it was a force pass outside a step (nbody_update_forces): its caller runs it again
            s.host_tree_once = true;
            return NBODY_OK;
        }
        s.elapsed = rest[0].elapsed_before;
        h->stats.steps -= rest.size();
        s.host_tree_once = true;             // (cleared by the force pass that uses it)
        int rc = s.sync_count(h, h->stream);
        if (rc) return rc;
        rc = step_end(h, rest[0].dt);         // forces on the host-built tree, kick + half drift
        if (rc) return rc;
        for (size_t k = 1; k < rest.size(); ++k) {
            rc = step_impl(h, rest[k].dt);    // (enqueued without read-back again: may poison again -> next round)
            if (rc) return rc;
        }
    }
    return fail(h, NBODY_ERR_INVALID, "resolve_async did not converge");
}

int step_begin(NbodyHandle* h, float dt) {
    State& s = *h->f32;
    if (!s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    nbody::launch_drift_half(h->stream, s.sh, int(s.n_local), dt, s.bnd);  // integrate_pre_force
    nbody::launch_compact(h->stream, s.sh, int(s.n_local));                 // retain
    s.count_dirty = true;
    HIP_TRY(h, hipGetLastError());
    if (nbody::tracer::on(h)) return nbody::tracer::drift_retain(h, dt);      // the same two on the tracer vector
    return NBODY_OK;
}

// update_forces up to (not including) whatever needs other GPUs' partial sums
int step_forces(NbodyHandle* h, float dt) {
    State& s = *h->f32;
    // an external field: no pass takes the kick along (they run as nbody_update_forces runs them); step_finish adds the field's
    // term to the finished accelerations and kicks
    const bool fuse = !nbody::ext::on(h);
    s.kick_pending = fuse;   // a force pass that ends in a plane reduction applies the kick itself
    s.kick_dt = dt;
    if (nbody::tracer::on(h) && h->cfg.method == NBODY_BRUTE_FORCE && !nbody::mesh::on(h)) {   // (mesh gravity: inside the pass, mesh_forces)
        // the tracers' force pass over the half-drifted, retained bodies, with the tracers' kick + half drift.  It reads the
        // bodies' positions and writes tracer state only, so it goes BEFORE the body pass, whose tail may move the bodies
        int rc = nbody::tracer::forces(h, fuse ? &s.kick_dt : nullptr);
        if (rc) { s.kick_pending = false; return rc; }
    }
    // (Barnes-Hut: the tracers walk the tree this pass builds, right after the bodies' walk: walk_tree)
    s.tracer_kick = fuse && nbody::tracer::on(h);
    int rc = forces_begin(h);                                                  // update_forces
    s.tracer_kick = false;
    if (rc) { s.kick_pending = false; s.tail_pending = false; }
    return rc;
}

int step_finish(NbodyHandle* h, float dt) {
    State& s = *h->f32;
    int rc = forces_finish(h);
    if (rc) { s.kick_pending = false; return rc; }
    if (nbody::ext::on(h)) {   // acc += s(x) at the half-drifted, retained positions, then integrate_after_force, bodies and tracers
        rc = nbody::ext::add(h, s.sh, s.n_local, s.g, &dt, true);
        if (!rc && nbody::tracer::on(h)) rc = nbody::ext::add(h, h->tr.sh, h->tr.n_host, s.g, &dt, false);
        if (rc) return rc;
    } else if (s.kick_pending) nbody::launch_kick_drift(h->stream, s.sh, int(s.n_local), dt);  // integrate_after_force
    s.kick_pending = false;
    HIP_TRY(h, hipGetLastError());
    if (h->ev_pending.size() >= 4096) {  // profiling left on over a long run: fold the timings in now and then
        rc = drain_events(h);
        if (rc) return rc;
    }
    s.elapsed += dt;                                                          // elapsed += dt
    h->stats.steps += 1;
    return NBODY_OK;
}

// what the grouped ncclSend/ncclRecv round delivers: the partial sums `peer` accumulated for this
// shard's bodies, into the plane reserved for that sender
int debug_import_partials(NbodyHandle* h, NbodyHandle* peer) {
    State& s = *h->f32;
    const State& ps = *peer->f32;
    if (!(s.cross_on && s.tail_pending)) return NBODY_OK;   // this force pass exchanges nothing
    if (!(ps.cross_on && ps.tail_pending)) return fail(h, NBODY_ERR_INVALID, "peer is not in the same phase");
    int src = -1, dst = -1;
    for (int i = 0; i < ps.cross.parts.n; ++i) if (ps.cross.parts.seg[i] == s.sh.my_seg) src = i;
    for (int i = 0; i < s.cross.n_recv; ++i) if (s.cross.recv_from[i] == ps.sh.my_seg) dst = i;
    if ((src < 0) != (dst < 0)) return fail(h, NBODY_ERR_INVALID, "send/receive plans of the two shards do not match");
    if (src < 0) return NBODY_OK;
    HIP_TRY(h, hipStreamSynchronize(peer->stream));
    HIP_TRY(h, hipMemcpyAsync(s.d_planes + size_t(s.recv_plane0 + dst) * s.sym_plan.plane_stride,
                              ps.d_send + size_t(src) * ps.sym_plan.plane_stride,
                              size_t(s.sh.seg_cap) * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}

int step_by(NbodyHandle* h, float dt) { return step_impl(h, dt); }

int steps(NbodyHandle* h, int k) {
    State& s = *h->f32;
    for (int i = 0; i < k; ++i) {
        int rc = step_impl(h, s.dt);  // Simulation::step, shared.rs:86-88
        if (rc) return rc;
    }
    return NBODY_OK;
}

int update_forces(NbodyHandle* h) {
    State& s = *h->f32;
    if (h->cfg.method == NBODY_BARNES_HUT && !s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    int rc = resolve_async(h);
    if (rc) return rc;
    rc = exchange_begin(h);
    if (rc) return rc;
    rc = forces(h);
    if (!rc && nbody::tracer::on(h) && h->cfg.method == NBODY_BRUTE_FORCE && !nbody::mesh::on(h)) rc = nbody::tracer::forces(h, nullptr);   // (Barnes-Hut: inside the pass, walk_tree; mesh gravity: mesh_forces)
    if (!rc && s.last_step_async) {
        s.last_step_async = false;
        rc = resolve_async(h);              // (a force pass outside a step is confirmed at once)
        if (!rc && s.host_tree_once) rc = forces(h);   // its build needed the host: once more, on the host-built tree
    }
    if (rc || !nbody::ext::on(h)) return rc;
    rc = nbody::ext::add<float>(h, s.sh, s.n_local, s.g, nullptr, false);   // acc += s(x), bodies and tracers
    if (!rc && nbody::tracer::on(h)) rc = nbody::ext::add<float>(h, h->tr.sh, h->tr.n_host, s.g, nullptr, false);
    return rc;
}

int stats(NbodyHandle* h, NbodyStats* out) { return engine::stats(h, *h->f32, out); }

int reset_stats(NbodyHandle* h) { return engine::reset_stats(h, *h->f32); }

int energy(NbodyHandle* h, double* kinetic, double* potential) {
    const int rc = resolve_async(h);
    return rc ? rc : engine::energy(h, *h->f32, kinetic, potential);
}

// nbody_potentials / nbody_energy_world on an f32 handle: S_i = sum m_j / sqrt(r2 + g_soft^2) of the own bodies into
// PotBufs::d_sum, at the CURRENT positions.  Index-block shards gather them first (in place: pos_all holds the other blocks
// as of mid-step, and the next step's exchange overwrites them again).  TREE mode runs the handle's own force pass -- host or
// device build, the same cells -- with PotBufs::walking set, so its last phase is the potential walk: accelerations, the
// walk counters and the force planes are not written.  The host's view of the body counts is put back as it was (engine::PotView).
// field = true (nbody_field_at): the same preparation with nothing summed over the bodies -- PAIRS: the gathered positions and
// live counts; TREE: the force pass up to its last phase, which leaves the tree and its split points in FieldBufs.
// (The mode and what a handle can take in it are checked by the caller: nbody_api.cpp potentials_device.)
int potentials_device(NbodyHandle* h, int mode, size_t* n_own, nbody::PotBodies* bodies, double* g, bool field) {
    if (h->let) return spatial_potentials(h, n_own, bodies, g);
    State& s = *h->f32;
    const bool tree = mode != NBODY_POTENTIAL_PAIRS, quad = mode == NBODY_POTENTIAL_TREE_QUADRUPOLE;
    if (tree && !s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    int rc = resolve_async(h);
    if (!rc) rc = exchange_wait(h);
    if (rc) return rc;
    if (s.sh.n_seg > 1) rc = engine::gather_blocks(h, s, h->stream);
    if (rc) return rc;
    engine::PotView<float> view(s);   // (the host's view of the counts: exact for the call, put back when it ends)
    const bool saved_once = s.host_tree_once;
    rc = view.begin(h, bodies, g);
    if (!rc && mode == NBODY_POTENTIAL_PAIRS) {
        const size_t n = s.n_local;
        if (!field) rc = nbody::pot::pairs(h, *bodies, n, total_upper(s) - n, double(s.g_soft) * double(s.g_soft));
    } else if (!rc) {
        PotWalkScope walking(h->pot, field ? kWalkField : kWalkPotentials, quad);
        const bool on_device = h->cfg.tree_build == NBODY_TREE_DEVICE;
        bool fell_back = false;
        if (on_device) rc = bh_walk_device_tree(h, &fell_back);
        if (!rc && (fell_back || !on_device)) rc = bh_walk_host_tree(h);   // (deeper than the device build goes: the host build, as the force pass does)
    }
    *n_own = s.n_local;
    s.host_tree_once = saved_once;
    return rc ? rc : comm_check(h);
}

int tree_export_quadrupoles(NbodyHandle* h, float* q6, size_t cap, size_t* n_nodes) {
    State& s = *h->f32;
    int rc = resolve_async(h);
    if (rc) return rc;
    const size_t n = s.tree.n_nodes;
    if (n_nodes) *n_nodes = n;
    if (!q6) return NBODY_OK;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "tree export buffer too small");
    if (n == 0) return NBODY_OK;
    // of the tree nbody_tree_export reports: the node array as it stands on the device (a tree call of nbody_potentials or
    // nbody_field_at since the force pass has rebuilt it), through the kernel the force pass runs
    HIP_TRY(h, grow_dev(h, h->d_quad, h->quad_cap, std::max(n, s.tree.node_cap), nbody::kQuadRecBytes, Grow::quarter));
    nbody::launch_tree_quad(h->stream, s.tree.d_nodes, int(n), h->d_quad, nullptr, nullptr);
    HIP_TRY(h, hipGetLastError());
    std::vector<float> rec(8 * n);
    HIP_TRY(h, hipMemcpyAsync(rec.data(), h->d_quad, n * nbody::kQuadRecBytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 6; ++k) q6[6 * i + k] = rec[8 * i + k];
    return NBODY_OK;
}

}  // namespace nbody32
