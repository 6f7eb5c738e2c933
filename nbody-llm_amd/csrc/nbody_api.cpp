// nbody_api.cpp -- the C ABI of include/nbody_hip.h: host orchestration of one shard.
//
// One handle = one reference `Simulation` object (src/shared.rs:80-97) living on one GPU.
// step_by follows brute_force.rs:84-90 / barnes_hut.rs:265-271 kernel by kernel:
//   K1 drift_half -> K4 compact (retain) -> [exchange] -> K2 | (host octree + K5) -> K3 kick_drift
// Everything is enqueued on the handle's own stream; the brute-force path never synchronises
// with the host inside nbody_steps, the Barnes-Hut path must (the octree is built on the host).
#include "nbody_handle.h"
#include "nbody_f64.h"
#include "nbody_let.h"
#include "nbody_pot.h"
#include "nbody_field.h"
#include "nbody_tracer.h"
#include "nbody_external.h"
#include "nbody_diag.h"
#include "nbody_pairs.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>


static thread_local std::string g_create_err;

int fail(NbodyHandle* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

namespace {

int use_device(NbodyHandle* h) {
    nbody::bind_tuning(&h->tune);   // the launchers below read this handle's knobs (kernels.h)
    HIP_TRY(h, hipSetDevice(h->device));
    return NBODY_OK;
}

size_t total_upper(const NbodyHandle* h) {
    size_t t = 0;
    for (int c : h->seg_count_host) t += size_t(c);
    return t;
}

// the once-per-step exchange of half-drifted positions: an in-place
// all-gather of the own segment into every rank's pos_all, plus the live counts
int exchange_begin(NbodyHandle* h) {
    if (h->sh.n_seg == 1 && !h->comm_ready) return NBODY_OK;  // (a 1-rank communicator still runs the collective)
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    // comm stream: after the drift/compaction of this step, beside whatever the compute stream does next
    HIP_TRY(h, hipEventRecord(h->ev_drifted, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->comm_stream, h->ev_drifted, 0));
    TP_TRY(h, h->tp->group_begin());
    TP_TRY(h, h->tp->all_gather(h->sh.pos_all, size_t(h->sh.seg_cap) * sizeof(float4), h->comm_stream));
    TP_TRY(h, h->tp->all_gather(h->sh.seg_count, sizeof(int), h->comm_stream));
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

// anything the transport noticed behind the host's back (a device-side wait that ran out of time, a peer that gave up)
int comm_check(NbodyHandle* h) {
    if (!h->tp) return NBODY_OK;
    int rc = h->tp->check();
    return rc ? fail(h, rc, h->tp->error()) : NBODY_OK;
}

int fail_if_hip(NbodyHandle* h, hipError_t e) { return e == hipSuccess ? NBODY_OK : fail(h, NBODY_ERR_HIP, hipGetErrorString(e)); }

// a record's stride holds the 10 F of a PointParticle<F,3> and keeps them aligned
int check_stride(NbodyHandle* h, size_t stride) {
    const size_t e = h->f64 ? sizeof(double) : sizeof(float);
    if (stride >= 10 * e && stride % e == 0) return NBODY_OK;
    return fail(h, NBODY_ERR_INVALID, h->f64 ? "f64 handle: stride must be a multiple of 8 and >= 80 bytes" : "stride must be a multiple of 4 and >= 40 bytes");
}

// ---- Vec::push / Vec::swap_remove on a world of index-block shards (collective: every rank makes the same call).
// The global vector is the concatenation of the ranks' blocks, so push appends to the LAST rank's block and
// swap_remove(i) moves the world's last body into slot i -- across ranks if they differ (one 40-byte message).
int sharded_counts_exact(NbodyHandle* h) {   // every rank learns every block's live count
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    int rc = exchange_wait(h);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    TP_TRY(h, h->tp->all_gather(h->sh.seg_count, sizeof(int), h->stream));
    h->count_dirty = true;
    return h->sync_count(h, h->stream);
}

int sharded_add_point(NbodyHandle* h, const void* particle) {
    int rc = sharded_counts_exact(h);
    if (rc) return rc;
    const int G = h->sh.n_seg, last = G - 1;
    if (total_upper(h) >= h->cfg.capacity || h->seg_count_host[last] >= h->sh.seg_cap)
        return fail(h, NBODY_ERR_CAPACITY, "capacity exhausted (a push goes to the end of the vector: the last rank's block is full)");
    // every rank raises its bound of the last block (its grids are sized from it; the device copy arrives with the next
    // exchange); the rank that owns the block does so by storing the body
    if (h->sh.my_seg == last) return h->push_one(h, h->stream, particle);
    h->seg_count_host[last] += 1;
    return NBODY_OK;
}

int sharded_remove_point(NbodyHandle* h, size_t index) {
    int rc = sharded_counts_exact(h);
    if (rc) return rc;
    const int G = h->sh.n_seg, me = h->sh.my_seg;
    if (index >= total_upper(h)) return fail(h, NBODY_ERR_INVALID, "swap_remove index out of range");   // Vec::swap_remove panics
    int r = 0, last = G - 1;
    size_t j = index;
    while (j >= size_t(h->seg_count_host[r])) { j -= size_t(h->seg_count_host[r]); ++r; }
    while (h->seg_count_host[last] == 0) --last;
    const size_t tail = size_t(h->seg_count_host[last]) - 1;   // the world's last body: (last, tail)
    if (r == last) {
        if (me == r && j != tail) {
            HIP_TRY(h, hipMemcpyAsync(h->sh.own_pos() + j, h->sh.own_pos() + tail, sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(h->sh.vel + j, h->sh.vel + tail, sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(h->sh.acc + j, h->sh.acc + tail, sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        }
    } else if (me == last || me == r) {
        rc = h->ensure_aos(h, 2);
        if (rc) return rc;
        if (me == last) {   // the world's last body as one PointParticle record, to the rank that holds slot `index`
            nbody::launch_soa_to_aos(h->stream, h->d_aos, 10, 1, h->sh.own_pos() + tail, h->sh.vel + tail, h->sh.acc + tail);
            TP_TRY(h, h->tp->send(h->d_aos, 40, r, h->stream));
        } else {
            TP_TRY(h, h->tp->recv(h->d_aos, 40, last, h->stream));
            nbody::launch_aos_to_soa(h->stream, h->d_aos, 10, 1, h->sh.own_pos() + j, h->sh.vel + j, h->sh.acc + j);
        }
        HIP_TRY(h, hipGetLastError());
    }
    if (me == last) {
        h->n_local = tail;
        rc = h->push_own_count(h, h->stream);
        if (rc) return rc;
    } else {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->seg_count_host[last] -= 1;
    return comm_check(h);
}

int drain_events(NbodyHandle* h) {
    if (h->ev_pending.empty()) return NBODY_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (auto& ev : h->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
            h->stats.force_kernel_ms += ms;
            h->stats.force_launches += 1;
        }
        h->ev_free.push_back(ev);
    }
    h->ev_pending.clear();
    return NBODY_OK;
}

constexpr size_t kShardedSymMinBodies = 2048; // sharded: own-own symmetric + remote one-sided from this size up

// (re)build the symmetric kernel's plan when the number of resident sets changes
int ensure_sym_plan(NbodyHandle* h) {
    const size_t set = size_t(64) * size_t(nbody::sym_bodies_per_lane(std::max<size_t>(1, h->n_local)));   // bodies of a resident set (make_sym_plan)
    const int A = int((std::max<size_t>(1, h->n_local) + set - 1) / set);  // (an empty shard still plans one set)
    const int knobs = nbody::tuning().sym_wpb * 100 + nbody::tuning().sym_rounds + nbody::tuning().sym_k * 10000 + nbody::tuning().sym_ipt * 1000000 + (nbody::tuning().sym_opp_rot ? 500000000 : 0);
    if (h->sym_plan.A == A && h->sym_plan.ipt * 64 == int(set) && h->d_sym_bounds && h->sym_waves == knobs) return NBODY_OK;
    h->sym_waves = knobs;
    h->sym_plan = nbody::make_sym_plan(int(std::max<size_t>(1, h->n_local)));
    nbody::SymPlan& p = h->sym_plan;
    h->cross_on = false;
    if (h->sh.n_seg > 1) {
        const size_t cap_pad = (size_t(h->sh.seg_cap) + 63) / 64 * 64;
        p.plane_stride = std::max(p.n_pad, cap_pad);
        if (nbody::tuning().cross_sym && h->sh.n_seg <= 2 * (nbody::CrossPartners::kMax - 1)) {
            // every unordered pair between shards once: this GPU is resident for some partners and
            // receives the partial sums the others accumulated for its bodies
            h->cross = nbody::make_cross_plan(h->sh.my_seg, h->sh.n_seg, h->sh.seg_cap, int(std::max<size_t>(1, h->n_local)));
            h->cross_on = true;
            h->recv_plane0 = p.n_planes + h->cross.k_res;
            p.n_planes += h->cross.k_res + h->cross.n_recv;
        } else {  // one-sided planes for the other shards' bodies: CU-sized 12-wave workgroups
            const int a_os = int((p.n_pad + 511) / 512);   // (k_bf_os keeps resident sets of 512 bodies whatever the symmetric kernel's are)
            p.k_os = std::max(1, std::min(256, 3072 / std::max(1, a_os)));
            p.plane_stride = std::max(p.plane_stride, size_t(a_os) * 512);   // (its padded lanes write their rows too)
            p.n_planes += p.k_os;
        }
    }
    // two cut tables of up to 127 entries: [0, 128) every set's, [128, 256) that of the sets that also meet their opposite set
    if (!h->d_sym_bounds) HIP_TRY(h, h->mem.dev(h->d_sym_bounds, 2 * 128 * sizeof(int)));
    HIP_TRY(h, hipMemcpyAsync(h->d_sym_bounds, p.bounds.data(), p.bounds.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_sym_bounds + 128, p.bounds_long.data(), p.bounds_long.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // p.bounds is pageable
    HIP_TRY(h, grow_dev(h, h->d_planes, h->planes_cap, size_t(p.n_planes) * p.plane_stride, sizeof(float4), Grow::exact));
    if (h->cross_on) {
        const nbody::CrossPlan& c = h->cross;
        if (c.slices.size() > h->cross_slices_cap)
            HIP_TRY(h, grow_dev(h, h->d_cross_slices, h->cross_slices_cap, c.slices.size() + 64, sizeof(int4), Grow::exact));
        if (!c.slices.empty()) {
            HIP_TRY(h, hipMemcpyAsync(h->d_cross_slices, c.slices.data(), c.slices.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        const size_t xneed = size_t(std::max(1, c.parts.n)) * size_t(c.A) * p.plane_stride;
        HIP_TRY(h, grow_dev(h, h->d_xplanes, h->xplanes_cap, xneed, sizeof(float4), Grow::exact));
        const size_t sneed = size_t(std::max(1, c.parts.n)) * p.plane_stride;
        HIP_TRY(h, grow_dev(h, h->d_send, h->send_cap, sneed, sizeof(float4), Grow::exact));
    }
    return NBODY_OK;
}

int bf_forces(NbodyHandle* h) {
    const float eps2 = h->g_soft * h->g_soft;  // brute_force.rs:69
    const bool fast = h->cfg.math_mode == NBODY_MATH_FAST && nbody::tuning().bf_fast_variant == 0;
    const bool sharded = h->sh.n_seg > 1;
    // Sharded: decided from the shard CAPACITY, which every rank shares.  The live counts differ from rank
    // to rank (ragged last block, bodies leaving the box), and a rank that chose another scheme than its
    // peers would neither send nor expect the partial sums the others exchange with it (a hang in RCCL).
    const bool sym = fast && (sharded ? size_t(h->sh.seg_cap) >= kShardedSymMinBodies : h->n_local >= size_t(std::max(1024, nbody::tuning().sym_min_bodies)));
    const size_t tot = total_upper(h);
    if (sym) {
        int rc = ensure_sym_plan(h);
        if (rc) return rc;
        if (h->sym_pairs_n != h->n_local) {
            h->sym_pairs = nbody::sym_main_pairs(h->sym_plan, h->n_local);
            h->sym_pairs_n = h->n_local;
        }
    }
    const nbody::SymPlan& p = h->sym_plan;
    uint64_t timed = 0;  // interactions of the launch the HIP events bracket (the dominant one)
    if (!(sym && sharded)) {
        int rc = exchange_wait(h);
        if (rc) return rc;
    }
    if (!sym) {
        ForceTimer t(h);
        if (h->cfg.math_mode == NBODY_MATH_STRICT) nbody::launch_bf_forces_strict(h->stream, h->sh, int(h->n_local), h->g, eps2);
        else nbody::launch_bf_forces_fast(h->stream, h->sh, int(h->n_local), h->g, eps2);
        timed = tot > 0 ? uint64_t(h->n_local) * uint64_t(tot - 1) : 0;
    } else if (!sharded) {
        {
            ForceTimer t(h);
            nbody::launch_bf_sym_main(h->stream, h->sh, p, h->d_sym_bounds, h->d_planes, int(h->n_local), eps2);
        }
        timed = 2 * h->sym_pairs;
        h->tail_pending = true;
    } else {
        // own shard symmetric (needs no remote data: it overlaps the exchange of positions) ...
        nbody::launch_bf_sym_main(h->stream, h->sh, p, h->d_sym_bounds, h->d_planes, int(h->n_local), eps2);
        {
            int rc = exchange_wait(h);
            if (rc) return rc;
        }
        if (h->cross_on) {
            // ... then the pairs with the partner shards, both sides; the partial sums for their bodies
            // go back to their owners before the planes are added up (forces_finish)
            const nbody::CrossPlan& c = h->cross;
            {
                ForceTimer t(h);
                nbody::launch_bf_cross(h->stream, h->sh, c, h->d_cross_slices,
                                       h->d_planes + size_t(h->recv_plane0 - c.k_res) * p.plane_stride, h->d_xplanes,
                                       h->d_send, p.plane_stride, eps2);
            }
            for (int i = 0; i < c.parts.n; ++i) {  // unordered pairs x 2, from the host's (upper-bound) counts
                const long long set = 64LL * c.ipt;
                const long long own = std::max(0LL, std::min<long long>(h->n_local, set * c.parts.a1[i]) - set * c.parts.a0[i]);
                const long long theirs = std::max(0LL, std::min<long long>(h->seg_count_host[c.parts.seg[i]], 64LL * c.parts.c1[i]) - 64LL * c.parts.c0[i]);
                timed += 2ull * uint64_t(own) * uint64_t(theirs);
            }
        } else {
            // ... then the other shards' bodies one-sided
            ForceTimer t(h);
            nbody::launch_bf_os(h->stream, h->sh, int((p.n_pad + 511) / 512), p.k_os, h->d_planes + size_t(p.n_planes - p.k_os) * p.plane_stride, p.plane_stride, eps2);
            timed = uint64_t(h->n_local) * uint64_t(tot - h->n_local);
        }
        h->tail_pending = true;
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
void free_all(NbodyHandle* h);
int resolve_async(NbodyHandle* h);
int step_end(NbodyHandle* h, float dt);
int step_impl(NbodyHandle* h, float dt);

// strict math with the reference leaf rule walks with the reference's nested sums (bit-exact): the store's per-lane stack, as
// many levels as the last tree is deep (the device build goes to 42; the host build reports its depth)
int setup_nested_walk(NbodyHandle* h, nbody::TreeDev* td) {
    if (h->cfg.math_mode != NBODY_MATH_STRICT || h->cfg.leaf_mode != NBODY_LEAF_REFERENCE) return NBODY_OK;
    int rc = h->tree.ensure_stack(h, h->sh.seg_cap, (h->tree.on_device ? 43 : h->tree.host.max_depth) + 2);
    if (rc) return rc;
    td->nested_stack = h->tree.d_stack;
    td->nested_stride = h->tree.stack_lanes;
    return NBODY_OK;
}

// fast math, variant 3: buffers of the LDS-staged walk and the threshold that picks the staged nodes.
// Called after this step's first host synchronisation, so h_hot_info holds the previous pass's flagged count.
int setup_lds_walk(NbodyHandle* h, nbody::TreeDev* td, size_t n_tree) {
#ifndef NBODY_TUNING
    (void)h; (void)td; (void)n_tree;   // (the experimental walks live in the tuning build)
    return NBODY_OK;
#else
    // (its stack holds the 42 levels of the device build; a deeper host-built tree is walked by k_bh_walk)
    if (h->cfg.math_mode == NBODY_MATH_FAST && nbody::tuning().bh_walk_variant == 5 && (h->tree.on_device || h->tree.host.max_depth <= 42)) {
        if (h->bfs_cap < h->tree.node_cap) {
            h->bfs_cap = 0;
            HIP_TRY(h, h->mem.dev(h->d_bfs, h->tree.node_cap * 2 * sizeof(float4)));
            HIP_TRY(h, h->mem.dev(h->d_bfs_ws, nbody::bfs_workspace_bytes(h->tree.node_cap)));
            h->bfs_cap = h->tree.node_cap;
        }
        td->bfs = h->d_bfs; td->bfs_ws = h->d_bfs_ws; td->bfs_cap = h->bfs_cap;
        return NBODY_OK;
    }
    if (h->cfg.math_mode != NBODY_MATH_FAST || nbody::tuning().bh_walk_variant != 3 || nbody::tuning().bh_hot_cap <= 0) return NBODY_OK;
    const int M = std::min(nbody::tuning().bh_hot_cap, 5000);  // 160 KB of LDS per CU, 32 B per record
    if (h->walk_cap < h->tree.node_cap) {
        h->walk_cap = 0;
        HIP_TRY(h, h->mem.dev(h->d_walk, (h->tree.node_cap + 1) * 2 * sizeof(float4)));
        HIP_TRY(h, h->mem.dev(h->d_unified, (h->tree.node_cap + 1) * sizeof(int)));
        h->walk_cap = h->tree.node_cap;
    }
    if (h->hot_cap != M) {
        h->hot_cap = 0;
        HIP_TRY(h, h->mem.dev(h->d_hot, size_t(M) * 2 * sizeof(float4)));
        HIP_TRY(h, hipMemsetAsync(h->d_hot, 0, size_t(M) * 2 * sizeof(float4), h->stream));
        h->hot_cap = M;
        h->hot_threshold_n = 0;
    }
    if (!h->d_hot_info) {
        HIP_TRY(h, h->mem.dev(h->d_hot_info, 2 * sizeof(int)));
        HIP_TRY(h, hipMemsetAsync(h->d_hot_info, 0, 2 * sizeof(int), h->stream));
        HIP_TRY(h, h->mem.pin(h->h_hot_info, 2 * sizeof(int)));
        h->h_hot_info[0] = h->h_hot_info[1] = 0;
    }
    if (h->hot_threshold_n == 0 || n_tree > 2 * h->hot_threshold_n || 2 * n_tree < h->hot_threshold_n) {
        // first guess: the grandparent holds 1/64 of the bodies (2 500 nodes at N = 65 536 Plummer)
        h->hot_threshold = int(std::max<size_t>(8, n_tree / 64));
        h->hot_threshold_n = std::max<size_t>(1, n_tree);
    } else {
        const int flagged = h->h_hot_info[1];
        if (flagged > M) h->hot_threshold = h->hot_threshold + h->hot_threshold / 8 + 1;
        else if (flagged < M - M / 3 && h->hot_threshold > 2) h->hot_threshold = h->hot_threshold - h->hot_threshold / 8 - 1;
    }
    td->walk = h->d_walk; td->unified = h->d_unified; td->hot = h->d_hot; td->hot_info = h->d_hot_info;
    td->hot_cap = M; td->hot_threshold = h->hot_threshold;
    return NBODY_OK;
#endif
}

// the cells' tensors from the node array as it now stands on the device (k_tree_quad), for the walk that follows
// (sized like the node array: a step without read-back knows its capacity only, and the build's node count on the device)
int fill_quadrupoles(NbodyHandle* h, const nbody::TreeDev& td, bool any_nodes) {
    HIP_TRY(h, grow_dev(h, h->d_quad, h->quad_cap, h->tree.node_cap, nbody::kQuadRecBytes, Grow::quarter));
    const bool counted_on_device = td.n_order_dev != nullptr;
    if (any_nodes) nbody::launch_tree_quad(h->stream, td.nodes, td.n_nodes, h->d_quad, counted_on_device ? h->tree.bufs.d_info : nullptr, td.poison);
    return NBODY_OK;
}

// the end of every f32 force pass: the buffers of the strict and the experimental walks, the walk over td (+ the kick and half
// drift when a step asked for them and the plane reduction can take them along)
int walk_tree(NbodyHandle* h, nbody::TreeDev& td, size_t n_tree) {
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
            nbody::launch_bh_pot_walk_quad(h->stream, h->sh.own_pos(), td, h->d_quad, h->g_soft * h->g_soft, h->theta2, h->pot.d_planes, stride,
                                           h->pot.d_sum, h->pot.d_counts);
        else
            nbody::launch_bh_pot_walk(h->stream, h->sh.own_pos(), td, h->g_soft * h->g_soft, h->theta2, h->pot.d_planes, stride, h->pot.d_sum,
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
        nbody::launch_bh_walk_quad(h->stream, h->sh, td, h->d_quad, h->g, h->g_soft * h->g_soft, h->theta2, h->d_counters,
                                   h->cfg.leaf_mode == NBODY_LEAF_DIRECT, h->kick_pending ? &h->kick_dt : nullptr, &kicked);
        if (kicked) h->kick_pending = false;
        HIP_TRY(h, hipGetLastError());
        return nbody::tracer::tree_forces(h, td);   // (tracers walk monopoles whatever the multipole setting)
    }
    int rc = setup_nested_walk(h, &td);
    if (!rc) rc = setup_lds_walk(h, &td, n_tree);
    if (rc) return rc;
    {
        ForceTimer t(h);
        int kicked = 0;
        nbody::launch_bh_walk(h->stream, h->sh, td, h->g, h->g_soft * h->g_soft, h->theta2,
                              h->cfg.math_mode == NBODY_MATH_FAST, h->d_counters, h->cfg.leaf_mode == NBODY_LEAF_DIRECT,
                              h->kick_pending ? &h->kick_dt : nullptr, &kicked);
        if (kicked) h->kick_pending = false;  // the plane reduction applied the kick + half drift
    }
    if (td.hot_cap > 0) HIP_TRY(h, hipMemcpyAsync(h->h_hot_info, h->d_hot_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipGetLastError());
    return nbody::tracer::tree_forces(h, td);   // the tracers' walk of the same tree, before anything overwrites it
}

// segments of the walk over the tree just built (a field call walks its probes, not the bodies)
int split_segments(const NbodyHandle* h, const TreeBuilt& t) {
    if (h->pot.walking == kWalkField) return field_split_plan(h->field.n_points, size_t(t.n_nodes));
    return walk_split_plan(t.n_order, h->cfg.math_mode != NBODY_MATH_STRICT || h->pot.walking, h->theta2, size_t(t.n_nodes)).segments;
}
// the walk over it, once the split points of its K segments are listed
int walk_built(NbodyHandle* h, const TreeBuilt& t, int K) {
    nbody::TreeDev td;
    td.nodes = h->tree.d_nodes; td.n_nodes = t.n_nodes;
    td.order = t.order; td.n_order = int(t.n_order);
    walk_split_view(h->tree.split, K, size_t(h->sh.seg_cap), &td);
    return walk_tree(h, td, t.n_tree);
}

int bh_forces(NbodyHandle* h) {
    {
        int rc = exchange_wait(h);
        if (rc) return rc;
    }
    h->last_step_async = false;
    if (h->cfg.tree_build == NBODY_TREE_DEVICE && !h->host_tree_once) {
        // no read-back at all: single shard, the plain or the strict walk (the experimental walks want the node count)
        const bool plain_walk = h->cfg.math_mode == NBODY_MATH_STRICT || nbody::tuning().bh_walk_variant == 0;
        if (h->async_bh && (plain_walk || h->multipole == NBODY_MULTIPOLE_QUADRUPOLE) && !nbody::tuning().bh_walk_debug) return bh_walk_device_tree_async(h);
        int rc = resolve_async(h);
        if (rc) return rc;
        bool fell_back = false;
        rc = bh_walk_device_tree(h, &fell_back);
        if (rc || !fell_back) return rc;
        // deeper than 42 levels somewhere: this step's tree comes from the host build below
    }
    h->host_tree_once = false;
    return bh_walk_host_tree(h);
}

// the force pass on the tree built on the host
int bh_walk_host_tree(NbodyHandle* h) {
    Shard& sh = h->sh;
    TreeBuilt t;
    int rc = h->tree.build_on_host(h, *h, &t);
    if (rc) return rc;
    // split the node range over several waves per body group when there are too few bodies to fill the chip (>= 8 waves per
    // SIMD wanted: the walk is bound by the latency of dependent loads).  ~3 waves per wave slot of the chip (256 CUs x 32),
    // handed out heaviest first (nbody::tuning().bh_walk_order): the launch lasts as long as its slowest wave, and smaller
    // pieces started in the right order shorten that tail (N = 65 536: 24 segments 0.310 ms, 8 segments 0.336 ms; tools/tune_bh_order.py)
    const int K = split_segments(h, t);
    rc = h->tree.split.ensure(h, K, size_t(sh.seg_cap));
    if (!rc) rc = h->tree.split.list_on_host(h, h->stream, h->tree.host.nodes, t.n_nodes, K);
    if (rc) return rc;
    return walk_built(h, t, K);
}

// Barnes-Hut force pass with the octree built on the device (kernels_tree.hip): no positions go to
// the host, no node array comes back; one 8-byte read-back (node count, flags) per step.
int bh_walk_device_tree(NbodyHandle* h, bool* fell_back) {
    TreeBuilt t;
    int rc = h->tree.build_on_device(h, *h, nbody::tuning().bh_walk_variant == 3, nullptr, &t);
    *fell_back = t.fell_back;
    if (rc || t.fell_back) return rc;
    const int K = split_segments(h, t);
    rc = h->tree.split.ensure(h, K, size_t(h->sh.seg_cap));
    if (rc) return rc;
    if (t.n_tree > 0) h->tree.split.list_on_device(h->stream, h->tree.work, int(t.n_tree), t.n_nodes, K);
    return walk_built(h, t, K);
}

// The same force pass with nothing read back: the node count, the live body count and the build's flags stay on the
// device (TreeBuildBufs::d_info); the split points are placed by k_tree_split_anc from the device's node count, the walk takes
// its body count from the device, and a build that needs the host poisons the run (see NbodyHandle::async_bh).
int bh_walk_device_tree_async(NbodyHandle* h) {
    Shard& sh = h->sh;
    auto t1 = clk::now();
    TreeBuildBufs& tb = h->tree.bufs;
    int rc = tb.ensure(h, size_t(sh.seg_cap), 0);
    if (rc) return rc;
    const size_t n_upper = h->n_local;   // an upper bound of the live count
    rc = h->tree.ensure_dev(h, TreeTypes<float>::kNodesPerBody * n_upper + 64, n_upper);
    if (rc) return rc;
    if (h->pending.empty()) HIP_TRY(h, hipMemsetAsync(h->d_poison + 1, 0, sizeof(int), h->stream));   // steps completed: counted from here
    // (a tree has at least as many nodes as bodies)
    const int K = walk_split_plan(n_upper, h->cfg.math_mode != NBODY_MATH_STRICT, h->theta2, n_upper).segments;
    rc = h->tree.split.ensure(h, K, size_t(sh.seg_cap));
    if (rc) return rc;
    // the walk's split points ride in the build's last launch (they also make a build that needs the host sticky: Shard::poison)
    const nbody::TreeSplitReq req = h->tree.split.request(K, tb.d_info, h->d_poison);
    nbody::TreeDevWork& work = h->tree.work;
    if (nbody::build_octree_device(h->stream, sh.own_pos(), sh.own_count(), int(n_upper), h->center, h->width, tb.ws, size_t(sh.seg_cap),
                                   h->tree.d_nodes, int(h->tree.node_cap), h->tree.d_order, tb.d_info, &work, 0, n_upper > 0 ? &req : nullptr) != 0)
        return fail(h, NBODY_ERR_HIP, "device octree build: rocPRIM call failed");
    HIP_TRY(h, hipGetLastError());
    h->stats.tree_build_ms += ms_since(t1);   // (enqueue time: nothing is waited for)
    h->tree.on_device = true;
    if (n_upper == 0)   // (no build was enqueued: the empty root's one segment, as a launch of its own)
        h->tree.split.list_on_device(h->stream, work, 0, int(h->tree.node_cap), K, tb.d_info, h->d_poison);
    nbody::TreeDev td;
    td.nodes = h->tree.d_nodes; td.n_nodes = int(h->tree.node_cap);   // (the plain walks end at the split points, not at n_nodes)
    td.order = h->tree.d_order; td.n_order = int(n_upper);
    td.n_order_dev = tb.d_info + 2;
    td.poison = h->d_poison;
    walk_split_view(h->tree.split, K, size_t(sh.seg_cap), &td);
    rc = walk_tree(h, td, n_upper);
    if (rc) return rc;
    h->last_step_async = true;
    h->count_dirty = true;
    return NBODY_OK;
}

// Where did the device get to?  Confirms the steps enqueued without read-back; if a build poisoned the run, finishes
// the failed step with the host build (which handles any depth) and enqueues the rest again.
int resolve_async(NbodyHandle* h) {
    if (!h->async_bh) return NBODY_OK;
    for (int round = 0; round < 1000000; ++round) {
        HIP_TRY(h, hipMemcpyAsync(h->h_poison, h->d_poison, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (h->tree.bufs.d_info) HIP_TRY(h, hipMemcpyAsync(h->h_poison + 2, h->tree.bufs.d_info, 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const int flags = h->h_poison[0], done = h->h_poison[1];
        if (!flags) {
            if (h->tree.on_device && h->tree.bufs.d_info) {   // what the last build produced
                h->tree.n_nodes = size_t(h->h_poison[2]);
                h->stats.tree_nodes = uint64_t(h->h_poison[2]);
            }
            h->pending.clear();
            return NBODY_OK;
        }
        // poisoned: steps [0, done) are complete, step `done` has drifted and compacted, nothing after it has run
        std::vector<NbodyHandle::PendingStep> rest;
        if (size_t(done) < h->pending.size()) rest.assign(h->pending.begin() + done, h->pending.end());
        h->pending.clear();
        HIP_TRY(h, hipMemsetAsync(h->d_poison, 0, 2 * sizeof(int), h->stream));
        if (flags & 2) {   // more nodes than the array holds: double it (the bound 4 n + 64 did not hold for this set)
            int rc = h->tree.ensure_dev(h, 2 * h->tree.node_cap + 64, h->n_local);
            if (rc) return rc;
        }
        if (rest.empty()) {   // it was a force pass outside a step (nbody_update_forces): its caller runs it again
            h->host_tree_once = true;
            return NBODY_OK;
        }
        h->elapsed = rest[0].elapsed_before;
        h->stats.steps -= rest.size();
        h->host_tree_once = true;             // (cleared by the force pass that uses it)
        int rc = h->sync_count(h, h->stream);
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

// ---- the partial sums other GPUs accumulated for the own bodies (symmetric scheme across shards)
int partials_begin(NbodyHandle* h) {
    if (!(h->cross_on && h->tail_pending) || h->cross.parts.n + h->cross.n_recv == 0) return NBODY_OK;
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    const nbody::CrossPlan& c = h->cross;
    const size_t S = h->sym_plan.plane_stride;
    const size_t bytes = size_t(h->sh.seg_cap) * sizeof(float4);
    HIP_TRY(h, hipEventRecord(h->ev_partials_ready, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->comm_stream, h->ev_partials_ready, 0));
    TP_TRY(h, h->tp->group_begin());
    for (int i = 0; i < c.parts.n; ++i)
        TP_TRY(h, h->tp->send(h->d_send + size_t(i) * S, bytes, c.parts.seg[i], h->comm_stream));
    for (int i = 0; i < c.n_recv; ++i)
        TP_TRY(h, h->tp->recv(h->d_planes + size_t(h->recv_plane0 + i) * S, bytes, c.recv_from[i], h->comm_stream));
    TP_TRY(h, h->tp->group_end());
    HIP_TRY(h, hipEventRecord(h->ev_partials_done, h->comm_stream));
    h->partials_in_flight = true;
    return NBODY_OK;
}

int partials_wait(NbodyHandle* h) {
    if (!h->partials_in_flight) return NBODY_OK;
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_partials_done, 0));
    h->partials_in_flight = false;
    return NBODY_OK;
}

// everything of the force pass that needs no other GPU's partial sums
int forces_begin(NbodyHandle* h) {
    return h->cfg.method == NBODY_BARNES_HUT ? bh_forces(h) : bf_forces(h);
}

// the plane reduction (with the kick + half drift when a step asked for it)
int forces_finish(NbodyHandle* h) {
    if (!h->tail_pending) return NBODY_OK;
    h->tail_pending = false;
    const float eps2 = h->g_soft * h->g_soft;
    nbody::launch_bf_sym_tail(h->stream, h->sh, h->sym_plan, h->d_planes, int(h->n_local), h->g, eps2,
                              h->kick_pending ? &h->kick_dt : nullptr);
    h->kick_pending = false;
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

int step_begin(NbodyHandle* h, float dt) {
    if (!h->bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    nbody::launch_drift_half(h->stream, h->sh, int(h->n_local), dt, h->bnd);  // integrate_pre_force
    nbody::launch_compact(h->stream, h->sh, int(h->n_local));                 // retain
    h->count_dirty = true;
    HIP_TRY(h, hipGetLastError());
    if (nbody::tracer::on(h)) return nbody::tracer::drift_retain(h, dt);      // the same two on the tracer vector
    return NBODY_OK;
}

// update_forces up to (not including) whatever needs other GPUs' partial sums
int step_forces(NbodyHandle* h, float dt) {
    // an external field: no pass takes the kick along (they run as nbody_update_forces runs them); step_finish adds the field's
    // term to the finished accelerations and kicks
    const bool fuse = !nbody::ext::on(h);
    h->kick_pending = fuse;   // a force pass that ends in a plane reduction applies the kick itself
    h->kick_dt = dt;
    if (nbody::tracer::on(h) && h->cfg.method == NBODY_BRUTE_FORCE) {
        // the tracers' force pass over the half-drifted, retained bodies, with the tracers' kick + half drift.  It reads the
        // bodies' positions and writes tracer state only, so it goes BEFORE the body pass, whose tail may move the bodies
        int rc = nbody::tracer::forces(h, fuse ? &h->kick_dt : nullptr);
        if (rc) { h->kick_pending = false; return rc; }
    }
    // (Barnes-Hut: the tracers walk the tree this pass builds, right after the bodies' walk: walk_tree)
    h->tr.kick_pending = fuse && nbody::tracer::on(h);
    int rc = forces_begin(h);                                                  // update_forces
    h->tr.kick_pending = false;
    if (rc) { h->kick_pending = false; h->tail_pending = false; }
    return rc;
}

int step_finish(NbodyHandle* h, float dt) {
    int rc = forces_finish(h);
    if (rc) { h->kick_pending = false; return rc; }
    if (nbody::ext::on(h)) {   // acc += s(x) at the half-drifted, retained positions, then integrate_after_force, bodies and tracers
        rc = nbody::ext::add(h, h->sh, h->n_local, h->g, &dt, true);
        if (!rc && nbody::tracer::on(h)) rc = nbody::ext::add(h, h->tr.sh, h->tr.n_host, h->g, &dt, false);
        if (rc) return rc;
    } else if (h->kick_pending) nbody::launch_kick_drift(h->stream, h->sh, int(h->n_local), dt);  // integrate_after_force
    h->kick_pending = false;
    HIP_TRY(h, hipGetLastError());
    if (h->ev_pending.size() >= 4096) {  // profiling left on over a long run: fold the timings in now and then
        rc = drain_events(h);
        if (rc) return rc;
    }
    h->elapsed += dt;                                                          // elapsed += dt
    h->stats.steps += 1;
    return NBODY_OK;
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
    const float elapsed_before = h->elapsed;
    int rc = step_begin(h, dt);
    if (rc) return rc;
    rc = exchange_begin(h);   // the force pass waits for it where it first needs remote bodies
    if (rc) return rc;
    rc = step_end(h, dt);
    if (rc) return rc;
    if (h->last_step_async) {   // nothing was read back: remember the step until the device's progress is confirmed
        h->pending.push_back(NbodyHandle::PendingStep{dt, elapsed_before});
        if (h->pending.size() >= 4096) rc = resolve_async(h);
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
    const int G = h->cfg.world_size, cap = h->sh.seg_cap;
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
    nbody::launch_pot_pack(ts, twin->sh.ids, twin->pot.d_sum, twin->sh.own_count(), cap, rec + size_t(h->cfg.rank) * size_t(cap));
    HIP_TRY(h, hipMemcpyAsync(p.d_rec_count + h->cfg.rank, twin->sh.own_count(), sizeof(int), hipMemcpyDeviceToDevice, ts));
    if (twin->comm_ready) {
        TP_TRY(twin, twin->tp->group_begin());
        TP_TRY(twin, twin->tp->all_gather(rec, size_t(cap) * sizeof(nbody::PotRec), ts));
        TP_TRY(twin, twin->tp->all_gather(p.d_rec_count, sizeof(int), ts));
        TP_TRY(twin, twin->tp->group_end());
    }
    HIP_TRY(h, hipMemsetAsync(p.d_slot_of, 0xFF, n_ids * sizeof(int), ts));
    nbody::launch_pot_scatter(ts, h->sh.ids, h->sh.own_count(), n_orig, p.d_slot_of, int(std::min<size_t>(n_ids, 0x7fffffff)), rec, p.d_rec_count, G, cap, p.d_sum);
    HIP_TRY(h, hipMemcpyAsync(p.d_counts, twin->pot.d_counts, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ts));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(ts));
    if (twin->tp) { rc = twin->tp->check(); if (rc) return fail(h, rc, twin->tp->error()); }
    return NBODY_OK;
}

int spatial_potentials(NbodyHandle* h, size_t* n_own, nbody::PotBodies* bodies, double* g) {
    if (!h->bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    if (h->cfg.world_size > 1 && !h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    const size_t saved_n = h->n_local;   // (nbody_clone refreshes the host's view of the count; the next walk's shape is drawn from the bound)
    const bool saved_dirty = h->count_dirty;
    const std::vector<int> saved_counts = h->seg_count_host;
    NbodyHandle* twin = nullptr;
    int rc = nbody_clone(h, &twin);
    const int n_orig = int(h->n_local);   // exact now
    h->n_local = saved_n; h->count_dirty = saved_dirty; h->seg_count_host = saved_counts;
    if (rc) return fail(h, rc, std::string("nbody_potentials: scratch clone: ") + nbody_last_error(nullptr));
    twin->tp = std::move(h->tp);          // the clones' world talks over this world's transport
    twin->comm_ready = h->comm_ready;
    nbody::bind_tuning(&twin->tune);
    rc = spatial_walk(h, twin, n_orig);
    if (rc && !twin->err.empty()) h->err = twin->err;
    h->tp = std::move(twin->tp);
    twin->comm_ready = false;
    nbody::bind_tuning(&h->tune);
    free_all(twin);
    (void)hipSetDevice(h->device);
    if (rc) return rc;
    bodies->pos_all = h->sh.pos_all; bodies->vel = h->sh.vel; bodies->seg_count = h->sh.seg_count;
    bodies->f64 = 0; bodies->n_seg = 1; bodies->seg_cap = h->sh.seg_cap; bodies->my_seg = 0;
    bodies->world = h->comm_ready ? h->cfg.world_size : 1;
    *g = double(h->g);
    *n_own = size_t(n_orig);
    return NBODY_OK;
}

// nbody_potentials / nbody_energy_world on an f32 handle: S_i = sum m_j / sqrt(r2 + g_soft^2) of the own bodies into
// PotBufs::d_sum, at the CURRENT positions.  Index-block shards gather them first (in place: pos_all holds the other blocks
// as of mid-step, and the next step's exchange overwrites them again).  TREE mode runs the handle's own force pass -- host or
// device build, the same cells -- with PotBufs::walking set, so its last phase is the potential walk: accelerations, the
// walk counters and the force planes are not written.  The host's view of the body counts is put back as it was: a step
// chain enqueued without read-back sizes its launches from the bound it has, and must do so with or without this call.
// field = true (nbody_field_at): the same preparation with nothing summed over the bodies -- PAIRS: the gathered positions and
// live counts; TREE: the force pass up to its last phase, which leaves the tree and its split points in FieldBufs.
// why this handle cannot take a call in NBODY_POTENTIAL_TREE_QUADRUPOLE (nullptr: it can)
const char* tree_quadrupole_refusal(const NbodyHandle* h) {
    if (h->cfg.method != NBODY_BARNES_HUT) return "this mode needs a Barnes-Hut handle (brute-force handles have no tree to expand)";
    if (h->f64 || h->cfg.dtype != NBODY_F32) return "this mode is not possible on NBODY_F64 handles (the cells' tensors exist for NBODY_F32)";
    if (h->let || h->cfg.shard_mode != NBODY_SHARD_INDEX) return "this mode is not possible on NBODY_SHARD_SPATIAL handles";
    if (h->cfg.world_size != 1) return "this mode is not possible on handles of a multi-rank world (world_size > 1)";
    return nullptr;
}

int potentials_device(NbodyHandle* h, int mode, size_t* n_own, nbody::PotBodies* bodies, double* g, bool field = false) {
    if (mode != NBODY_POTENTIAL_PAIRS && mode != NBODY_POTENTIAL_TREE && mode != NBODY_POTENTIAL_TREE_QUADRUPOLE)
        return fail(h, NBODY_ERR_INVALID, "mode must be NBODY_POTENTIAL_PAIRS, NBODY_POTENTIAL_TREE or NBODY_POTENTIAL_TREE_QUADRUPOLE");
    const bool quad = mode == NBODY_POTENTIAL_TREE_QUADRUPOLE;
    if (quad)
        if (const char* why = tree_quadrupole_refusal(h)) return fail(h, NBODY_ERR_INVALID, std::string("NBODY_POTENTIAL_TREE_QUADRUPOLE: ") + why);
    const bool tree = mode != NBODY_POTENTIAL_PAIRS;
    if (h->let && field)
        return fail(h, NBODY_ERR_INVALID, "nbody_field_at is not possible on NBODY_SHARD_SPATIAL handles: a rank holds neither the world's bodies nor the tree around a foreign point");
    if (h->let && mode == NBODY_POTENTIAL_PAIRS)
        return fail(h, NBODY_ERR_INVALID, "NBODY_POTENTIAL_PAIRS is not possible on NBODY_SHARD_SPATIAL handles (a rank does not hold the world's bodies): NBODY_POTENTIAL_TREE is the mode for them");
    if (h->let) return spatial_potentials(h, n_own, bodies, g);
    if (tree && h->cfg.method != NBODY_BARNES_HUT) return fail(h, NBODY_ERR_INVALID, "NBODY_POTENTIAL_TREE needs a Barnes-Hut handle");
    if (h->f64) return nbody64::potentials_device(h, mode, n_own, bodies, g, field);
    if (tree && !h->bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    Shard& sh = h->sh;
    int rc = resolve_async(h);
    if (!rc) rc = exchange_wait(h);
    if (rc) return rc;
    if (sh.n_seg > 1) {
        if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
        TP_TRY(h, h->tp->group_begin());
        TP_TRY(h, h->tp->all_gather(sh.pos_all, size_t(sh.seg_cap) * sizeof(float4), h->stream));
        TP_TRY(h, h->tp->all_gather(sh.seg_count, sizeof(int), h->stream));
        TP_TRY(h, h->tp->group_end());
    }
    const size_t saved_n = h->n_local;
    const bool saved_dirty = h->count_dirty, saved_once = h->host_tree_once;
    const std::vector<int> saved_counts = h->seg_count_host;
    h->count_dirty = true;
    rc = h->sync_count(h, h->stream);
    if (!rc) rc = nbody::pot::begin(h, size_t(sh.seg_cap));
    bodies->pos_all = sh.pos_all; bodies->vel = sh.vel; bodies->seg_count = sh.seg_count;
    bodies->f64 = 0; bodies->n_seg = sh.n_seg; bodies->seg_cap = sh.seg_cap; bodies->my_seg = sh.my_seg;
    bodies->world = sh.n_seg;
    *g = double(h->g);
    if (!rc && mode == NBODY_POTENTIAL_PAIRS) {
        const size_t n = h->n_local;
        if (!field) rc = nbody::pot::pairs(h, *bodies, n, total_upper(h) - n, double(h->g_soft) * double(h->g_soft));
    } else if (!rc) {
        PotWalkScope walking(h->pot, field ? kWalkField : kWalkPotentials, quad);
        const bool on_device = h->cfg.tree_build == NBODY_TREE_DEVICE;
        bool fell_back = false;
        if (on_device) rc = bh_walk_device_tree(h, &fell_back);
        if (!rc && (fell_back || !on_device)) rc = bh_walk_host_tree(h);   // (deeper than the device build goes: the host build, as the force pass does)
    }
    *n_own = h->n_local;
    h->n_local = saved_n; h->count_dirty = saved_dirty; h->seg_count_host = saved_counts; h->host_tree_once = saved_once;
    if (rc) return rc;
    return comm_check(h);
}

void free_all(NbodyHandle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    h->tp.reset();   // (leaves the world: the ipc transport waits, bounded, until its peers are done with its window)
    if (h->ev_drifted) (void)hipEventDestroy(h->ev_drifted);
    if (h->ev_gathered) (void)hipEventDestroy(h->ev_gathered);
    if (h->ev_partials_ready) (void)hipEventDestroy(h->ev_partials_ready);
    if (h->ev_partials_done) (void)hipEventDestroy(h->ev_partials_done);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    for (auto& ev : h->ev_pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (auto& ev : h->ev_free) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    nbody64::destroy(h);      // (the states and their events; their memory is the registry's like everything else)
    nbody::let::destroy(h);
    h->tree.host.clear();     // (the host octree's pinned node arrays are its own: nbody_handle.h pinned_alloc)
    h->mem.release_all();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int create_impl(const NbodyConfig* cfg, NbodyHandle** out) {
    if (!cfg || !out) return fail(nullptr, NBODY_ERR_INVALID, "null argument");
    // ABI versions <= 2 end before shard_mode (48 bytes): such a caller gets index-block shards
    constexpr uint32_t kOldConfigSize = 48;
    NbodyConfig full{};
    if (cfg->struct_size == kOldConfigSize) { std::memcpy(&full, cfg, kOldConfigSize); full.struct_size = sizeof(NbodyConfig); cfg = &full; }
    if (cfg->struct_size != sizeof(NbodyConfig)) return fail(nullptr, NBODY_ERR_INVALID, "NbodyConfig.struct_size mismatch");
    if (cfg->shard_mode != NBODY_SHARD_INDEX && cfg->shard_mode != NBODY_SHARD_SPATIAL) return fail(nullptr, NBODY_ERR_INVALID, "unknown shard_mode");
    if (cfg->shard_mode == NBODY_SHARD_SPATIAL && (cfg->method != NBODY_BARNES_HUT || cfg->math_mode != NBODY_MATH_FAST || cfg->dtype != NBODY_F32))
        return fail(nullptr, NBODY_ERR_INVALID, "NBODY_SHARD_SPATIAL is the fast-math f32 Barnes-Hut path (halo exchange over the device-built tree)");
    if (cfg->method != NBODY_BRUTE_FORCE && cfg->method != NBODY_BARNES_HUT) return fail(nullptr, NBODY_ERR_INVALID, "unknown method");
    if (cfg->math_mode != NBODY_MATH_STRICT && cfg->math_mode != NBODY_MATH_FAST) return fail(nullptr, NBODY_ERR_INVALID, "unknown math_mode");
    if (cfg->leaf_mode != NBODY_LEAF_REFERENCE && cfg->leaf_mode != NBODY_LEAF_DIRECT) return fail(nullptr, NBODY_ERR_INVALID, "unknown leaf_mode");
    if (cfg->tree_build != NBODY_TREE_HOST && cfg->tree_build != NBODY_TREE_DEVICE && cfg->tree_build != NBODY_TREE_AUTO)
        return fail(nullptr, NBODY_ERR_INVALID, "unknown tree_build");
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail(nullptr, NBODY_ERR_INVALID, "bad rank/world_size");
    if (cfg->capacity == 0 || cfg->capacity > (1ull << 30)) return fail(nullptr, NBODY_ERR_INVALID, "capacity must be in [1, 2^30]");
    if (cfg->dtype != NBODY_F32 && cfg->dtype != NBODY_F64) return fail(nullptr, NBODY_ERR_INVALID, "unknown dtype");
    if (cfg->dtype == NBODY_F64 && cfg->world_size != 1 && cfg->shard_mode != NBODY_SHARD_INDEX)
        return fail(nullptr, NBODY_ERR_INVALID, "f64 worlds are sharded by index blocks (NBODY_SHARD_INDEX)");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, NBODY_ERR_NO_DEVICE, "no HIP device (this library has no CPU fallback)");
    int dev = cfg->device;
    if (dev < 0) {
        const char* lr = std::getenv("LOCAL_RANK");
        dev = lr ? std::atoi(lr) % ndev : 0;
    }
    if (dev >= ndev) return fail(nullptr, NBODY_ERR_INVALID, "device ordinal out of range");

    NbodyHandle* h = new NbodyHandle();
    h->cfg = *cfg;
    if (h->cfg.tree_build == NBODY_TREE_AUTO)   // the bit-exact path keeps the reference's (host) build
        h->cfg.tree_build = cfg->math_mode == NBODY_MATH_FAST ? NBODY_TREE_DEVICE : NBODY_TREE_HOST;
    if (h->cfg.dtype == NBODY_F64) {
        // F = f64: brute force strict = the reference's loop (k_bf_strict, bit-exact), fast = every unordered pair once
        // (kernels_bf64.hip); Barnes-Hut strict = the reference's nested sums on the host-built tree (bit-exact) unless the
        // device build is asked for, fast = one running sum per lane over a split node range, on the device-built tree
        // unless the host build is asked for (AUTO: as for f32)
        if (cfg->tree_build == NBODY_TREE_AUTO) h->cfg.tree_build = h->cfg.math_mode == NBODY_MATH_FAST ? NBODY_TREE_DEVICE : NBODY_TREE_HOST;
        if (cfg->world_size > 1 && h->cfg.math_mode != NBODY_MATH_FAST) h->cfg.tree_build = NBODY_TREE_HOST;   // (a sharded f64 world in strict math builds the replicated tree on the host; fast math: on the device, from the gathered positions)
    }
    if (h->cfg.shard_mode == NBODY_SHARD_SPATIAL) h->cfg.tree_build = NBODY_TREE_DEVICE;
    cfg = &h->cfg;
    h->device = dev;
    *out = nullptr;
    auto bail = [&](int rc) { g_create_err = h->err; free_all(h); return rc; };
#define CREATE_TRY(expr)                                                                                  \
    do {                                                                                                  \
        const int rc_ = [&] { HIP_TRY(h, expr); return int(NBODY_OK); }();                                \
        if (rc_) return bail(rc_);                                                                        \
    } while (0)
    CREATE_TRY(hipSetDevice(dev));
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CREATE_TRY(h->mem.pin(h->h_poison, 8 * sizeof(int)));
    if (cfg->method == NBODY_BARNES_HUT) {
        // default: the cores this process may run on, at most 16 (a GPU's share of the host; more
        // threads than top-level subtrees only add wake-up latency)
        int threads = cfg->host_threads > 0 ? cfg->host_threads : std::min(16, std::max(1, int(std::thread::hardware_concurrency()) - 2));
        h->pool.reset(new nbody::WorkerPool(std::max(1, threads)));
        CREATE_TRY(h->mem.dev(h->d_counters, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long)));
        CREATE_TRY(hipMemsetAsync(h->d_counters, 0, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), h->stream));
        CREATE_TRY(h->mem.pin(h->h_counters, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long)));
    }
    Shard& sh = h->sh;
    sh.n_seg = cfg->world_size;
    sh.my_seg = cfg->rank;
    sh.seg_cap = int((cfg->capacity + cfg->world_size - 1) / cfg->world_size);   // bodies an index block can hold
    if (cfg->dtype == NBODY_F64) {   // the bodies of an f64 handle live in nbody64::State (this store keeps the shape only)
        h->seg_count_host.assign(size_t(sh.n_seg), 0);
        int rc64 = nbody64::create(h);
        if (rc64) return bail(rc64);
        *out = h;
        return NBODY_OK;
    }
    const bool spatial = cfg->shard_mode == NBODY_SHARD_SPATIAL;
    if (spatial) {   // a spatial handle holds its own bodies only (no gathered positions): one segment, with room for immigrants
        sh.n_seg = 1;
        sh.my_seg = 0;
        // (four times the even share: the bounds equalise the ranks' WORK, and a rank of cheap bodies -- a sparse halo --
        // owns more than the average; NBODY_ERR_CAPACITY beyond that)
        if (cfg->world_size > 1) sh.seg_cap = int(std::min<uint64_t>(cfg->capacity, 4 * uint64_t(sh.seg_cap) + 64));
    }
    {
        int rc = h->alloc(h, h->stream);
        if (rc) return bail(rc);
    }
    CREATE_TRY(h->mem.dev(h->d_poison, 2 * sizeof(int)));
    CREATE_TRY(hipMemsetAsync(h->d_poison, 0, 2 * sizeof(int), h->stream));
    if (cfg->method == NBODY_BARNES_HUT) {
        int rc = h->tree.alloc_host(h, sh);
        if (rc) return bail(rc);
    }
    CREATE_TRY(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
    {
        const char* v = std::getenv("NBODY_BH_ASYNC");
        h->async_bh = cfg->method == NBODY_BARNES_HUT && cfg->tree_build == NBODY_TREE_DEVICE && cfg->world_size == 1 &&
                      !spatial && !(v && v[0] == '0');
        if (h->async_bh) sh.poison = h->d_poison;
    }
    if (spatial) {
        int rc_let = nbody::let::create(h);
        if (rc_let) return bail(rc_let);
    }
    {   // the documented environment switches set this handle's knobs (nbody_set_tuning changes them later)
        nbody::Tuning& t = h->tune;
        const struct { const char* env; int* knob; } table[] = {
            {"NBODY_BF_VARIANT", &t.bf_fast_variant}, {"NBODY_CROSS_SYM", &t.cross_sym}, {"NBODY_SYM_PACKED", &t.sym_packed},
            {"NBODY_BH_SPLIT", &t.bh_walk_split}, {"NBODY_SYM_WPB", &t.sym_wpb}, {"NBODY_SYM_IPT", &t.sym_ipt}, {"NBODY_BH_DUO", &t.bh_walk_duo}, {"NBODY_BH_XCD", &t.bh_walk_xcd},
#ifdef NBODY_TUNING
            {"NBODY_BH_VARIANT", &t.bh_walk_variant}, {"NBODY_BH_HOT", &t.bh_hot_cap}, {"NBODY_BH_LDS_BLOCK", &t.bh_walk_lds_block},
#endif
        };
        for (const auto& e : table)
            if (const char* v = std::getenv(e.env)) *e.knob = std::atoi(v);
    }
    *out = h;
    return NBODY_OK;
}

}  // namespace

// =============================================================================== C entry points
extern "C" {

int nbody_abi_version(void) { return NBODY_ABI_VERSION; }

int nbody_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* nbody_last_error(const NbodyHandle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int nbody_create(const NbodyConfig* cfg, NbodyHandle** out) { return create_impl(cfg, out); }

void nbody_destroy(NbodyHandle* h) { free_all(h); }

int nbody_clone(const NbodyHandle* src, NbodyHandle** out) {
    if (!src || !out) return fail(nullptr, NBODY_ERR_INVALID, "null argument");
    NbodyHandle* s = const_cast<NbodyHandle*>(src);
    int rc = use_device(s);
    if (rc) return rc;
    rc = resolve_async(s);
    if (rc) return rc;
    if (!s->f64) rc = s->sync_count(s, s->stream);
    if (rc) return rc;
    NbodyHandle* h = nullptr;
    rc = create_impl(&src->cfg, &h);
    if (rc) return rc;
    h->tune = src->tune;   // (the knobs shape the fast passes' sums: a clone continues bit for bit like its source)
    h->ext = src->ext;     // (and the external field)
    if (src->f64) {
        rc = nbody64::clone_state(s, h);
        if (rc) { g_create_err = h->err; free_all(h); return rc; }
        *out = h;
        return NBODY_OK;
    }
    rc = fail_if_hip(h, hipStreamSynchronize(s->stream));
    if (!rc) rc = h->copy_from(h, h->stream, *src);
    if (!rc) rc = fail_if_hip(h, hipStreamSynchronize(h->stream));
    if (rc) { g_create_err = "clone copy: " + h->err; free_all(h); return rc; }
    h->multipole = src->multipole;
    h->first_global = src->first_global; h->n_at_upload = src->n_at_upload;
    if (src->let) {   // spatial shards: + the bodies' ids and the ownership bounds
        rc = nbody::let::clone_state(s, h);
        if (rc) { g_create_err = h->err; free_all(h); return rc; }
    }
    rc = nbody::tracer::clone_state(s, h);
    if (rc) { g_create_err = h->err; free_all(h); return rc; }
    // like the reference's BH clone (barnes_hut.rs:113-135) the tree is not carried over; neither
    // are the communicator (call nbody_comm_init on the clone) and the statistics
    *out = h;
    return NBODY_OK;
}

int nbody_upload(NbodyHandle* h, const void* aos, size_t n, size_t stride) {
    if (!h || (!aos && n)) return fail(h, NBODY_ERR_INVALID, "null argument");
    int rc = check_stride(h, stride);
    if (rc) return rc;
    if (n > h->cfg.capacity) return fail(h, NBODY_ERR_CAPACITY, "more bodies than NbodyConfig.capacity");
    rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::upload(h, aos, n, stride);
    if (h->let) return nbody::let::upload(h, aos, n, stride);
    rc = resolve_async(h);
    if (rc) return rc;
    rc = h->upload_blocks(h, h->stream, aos, n, stride, &h->first_global);
    h->n_at_upload = h->n_local;
    return rc;
}

int nbody_download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = check_stride(h, stride);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::download(h, aos, cap, stride, n_out);
    rc = resolve_async(h);
    if (rc) return rc;
    return h->download_own(h, h->stream, aos, cap, stride, n_out, comm_check);   // (bodies of a run whose exchange broke down are not handed out as results)
}

int nbody_count(NbodyHandle* h, size_t* n_out) {
    if (!h || !n_out) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::count(h, n_out);
    rc = resolve_async(h);
    if (rc) return rc;
    rc = h->sync_count(h, h->stream);
    if (rc) return rc;
    *n_out = h->n_local;
    return NBODY_OK;
}

int nbody_count_global(NbodyHandle* h, size_t* n_out) {
    if (!h || !n_out) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::count_global(h, n_out);
    if (h->let) return nbody::let::count_global(h, n_out);
    rc = resolve_async(h);
    if (rc) return rc;
    rc = h->sync_count(h, h->stream);
    if (rc) return rc;
    *n_out = total_upper(h);
    return NBODY_OK;
}

int nbody_add_point(NbodyHandle* h, const void* particle) {
    if (!h || !particle) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::add_point(h, particle);
    if (h->let) return nbody::let::add_point(h, particle);
    if (h->sh.n_seg != 1) return sharded_add_point(h, particle);
    rc = resolve_async(h);
    if (rc) return rc;
    return h->push_one(h, h->stream, particle);
}

int nbody_remove_point(NbodyHandle* h, size_t index) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::remove_point(h, index);
    if (h->let) return nbody::let::remove_point(h, index);
    if (h->sh.n_seg != 1) return sharded_remove_point(h, index);
    rc = resolve_async(h);
    if (rc) return rc;
    return h->swap_remove_one(h, h->stream, index);
}

int nbody_set_settings_f64(NbodyHandle* h, double g, double g_soft, double dt, double theta2) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->f64) return nbody64::set_settings(h, g, g_soft, dt, theta2);
    h->set_settings(float(g), float(g_soft), float(dt), float(theta2));
    return NBODY_OK;
}

int nbody_set_settings(NbodyHandle* h, float g, float g_soft, float dt, float theta2) {
    return nbody_set_settings_f64(h, double(g), double(g_soft), double(dt), double(theta2));   // (f32 -> f64 -> f32 is exact)
}

int nbody_get_settings_f64(const NbodyHandle* h, double* g, double* g_soft, double* dt, double* theta2) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->f64) return nbody64::get_settings(h, g, g_soft, dt, theta2);
    h->get_settings(g, g_soft, dt, theta2);
    return NBODY_OK;
}

int nbody_get_settings(const NbodyHandle* h, float* g, float* g_soft, float* dt, float* theta2) {
    if (!h) return NBODY_ERR_INVALID;
    if (!h->f64) { h->get_settings(g, g_soft, dt, theta2); return NBODY_OK; }
    double v[4];
    nbody64::get_settings(h, &v[0], &v[1], &v[2], &v[3]);
    if (g) *g = float(v[0]);
    if (g_soft) *g_soft = float(v[1]);
    if (dt) *dt = float(v[2]);
    if (theta2) *theta2 = float(v[3]);
    return NBODY_OK;
}

int nbody_set_bounds_f64(NbodyHandle* h, const double center[3], double width) {
    if (!h || !center) return NBODY_ERR_INVALID;
    if (h->f64) return nbody64::set_bounds(h, center, width);
    const float c[3] = {float(center[0]), float(center[1]), float(center[2])};
    h->set_bounds(c, float(width));
    return NBODY_OK;
}

int nbody_set_bounds(NbodyHandle* h, const float center[3], float width) {
    if (!h || !center) return NBODY_ERR_INVALID;
    const double c[3] = {double(center[0]), double(center[1]), double(center[2])};
    return nbody_set_bounds_f64(h, c, double(width));   // (f32 -> f64 -> f32 is exact)
}

int nbody_init(NbodyHandle* h) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->f64) return nbody64::init(h);
    h->elapsed = 0.f;  // brute_force.rs:49; the reference's BH init also builds a tree that the
                       // first update_forces rebuilds before any use (barnes_hut.rs:232-235, 251-254)
    return NBODY_OK;
}

int nbody_step_by(NbodyHandle* h, float dt) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::step_by(h, double(dt));
    if (h->let) return nbody::let::step(h, dt);
    return step_impl(h, dt);
}

int nbody_step_by_f64(NbodyHandle* h, double dt) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::step_by(h, dt);
    if (h->let) return nbody::let::step(h, float(dt));
    return step_impl(h, float(dt));
}

int nbody_steps(NbodyHandle* h, int k) {
    if (!h || k < 0) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::steps(h, k);
    if (h->let) {
        for (int i = 0; i < k; ++i) { rc = nbody::let::step(h, h->dt); if (rc) return rc; }
        return NBODY_OK;
    }
    for (int i = 0; i < k; ++i) {
        rc = step_impl(h, h->dt);  // Simulation::step, shared.rs:86-88
        if (rc) return rc;
    }
    return NBODY_OK;
}

int nbody_update_forces(NbodyHandle* h) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::update_forces(h);
    if (h->let) return h->bounds_set ? nbody::let::update_forces(h) : fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    if (h->cfg.method == NBODY_BARNES_HUT && !h->bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    rc = resolve_async(h);
    if (rc) return rc;
    rc = exchange_begin(h);
    if (rc) return rc;
    rc = forces(h);
    if (!rc && nbody::tracer::on(h) && h->cfg.method == NBODY_BRUTE_FORCE) rc = nbody::tracer::forces(h, nullptr);   // (Barnes-Hut: inside the pass, walk_tree)
    if (!rc && h->last_step_async) {
        h->last_step_async = false;
        rc = resolve_async(h);              // (a force pass outside a step is confirmed at once)
        if (!rc && h->host_tree_once) rc = forces(h);   // its build needed the host: once more, on the host-built tree
    }
    if (rc || !nbody::ext::on(h)) return rc;
    rc = nbody::ext::add<float>(h, h->sh, h->n_local, h->g, nullptr, false);   // acc += s(x), bodies and tracers
    if (!rc && nbody::tracer::on(h)) rc = nbody::ext::add<float>(h, h->tr.sh, h->tr.n_host, h->g, nullptr, false);
    return rc;
}

// ---- the static external field (nbody_external.cpp)
namespace {
// binds the device, refuses the handles that take no field, naming the entry point, and confirms the steps enqueued without a
// read-back: they were asked for under the field as it stood, and the readers want the positions they produced
int external_enter(NbodyHandle* h, const char* call) {
    int rc = use_device(h);
    if (rc) return rc;
    if (const char* why = nbody::ext::refusal(h)) return fail(h, NBODY_ERR_INVALID, std::string(call) + ": " + why);
    return resolve_async(h);
}
double g_of(const NbodyHandle* h) {
    double g = double(h->g);
    if (h->f64) nbody64::get_settings(h, &g, nullptr, nullptr, nullptr);
    return g;
}
// per body potentials (phi may be null) and sum m phi (energy may be null) at the current positions; *n_out = live bodies
int external_potentials(NbodyHandle* h, bool want_phi, double* phi, size_t cap, size_t* n_out, double* energy, const char* call) {
    size_t n = 0;
    int rc = NBODY_OK;
    if (h->f64) rc = nbody64::count(h, &n);
    else { rc = h->sync_count(h, h->stream); n = h->n_local; }
    if (rc) return rc;
    if (n_out) *n_out = n;
    if (want_phi && n > cap) return fail(h, NBODY_ERR_CAPACITY, std::string(call) + ": buffer too small");
    if (want_phi && n && !phi) return fail(h, NBODY_ERR_INVALID, std::string(call) + ": phi is NULL");
    if (h->f64) return nbody::ext::potentials(h, nbody64::shard(h), n, g_of(h), phi, energy);
    return nbody::ext::potentials(h, h->sh, n, g_of(h), phi, energy);
}
}  // namespace

int nbody_set_external_field(NbodyHandle* h, const NbodyExternalComponent* comps, size_t n) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = external_enter(h, "nbody_set_external_field");
    if (rc) return rc;
    const std::string why = nbody::ext::invalid(comps, n, !h->f64);
    if (!why.empty()) return fail(h, NBODY_ERR_INVALID, "nbody_set_external_field: " + why);
    if (n > 0 && h->f64 && nbody64::get_integrator(h) == NBODY_INTEGRATOR_HERMITE4)
        return fail(h, NBODY_ERR_INVALID, "nbody_set_external_field: the handle runs the Hermite integrator, which would need the field's jerk (out of scope)");
    h->ext = ExternalField{};
    h->ext.n = int(n);
    std::copy(comps, comps + n, h->ext.given);
    return NBODY_OK;
}

int nbody_get_external_field(const NbodyHandle* h, NbodyExternalComponent* comps, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    NbodyHandle* hh = const_cast<NbodyHandle*>(h);
    if (const char* why = nbody::ext::refusal(h)) return fail(hh, NBODY_ERR_INVALID, std::string("nbody_get_external_field: ") + why);
    const size_t n = size_t(h->ext.n);
    if (n_out) *n_out = n;
    if (n > cap) return fail(hh, NBODY_ERR_CAPACITY, "nbody_get_external_field: buffer too small");
    if (n && !comps) return fail(hh, NBODY_ERR_INVALID, "nbody_get_external_field: comps is NULL");
    std::copy(h->ext.given, h->ext.given + n, comps);
    return NBODY_OK;
}

int nbody_external_potentials(NbodyHandle* h, double* phi, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = external_enter(h, "nbody_external_potentials");
    if (rc) return rc;
    return external_potentials(h, true, phi, cap, n_out, nullptr, "nbody_external_potentials");
}

int nbody_external_energy(NbodyHandle* h, double* potential) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = external_enter(h, "nbody_external_energy");
    if (rc) return rc;
    if (!potential) return fail(h, NBODY_ERR_INVALID, "nbody_external_energy: potential is NULL");
    return external_potentials(h, false, nullptr, 0, nullptr, potential, "nbody_external_energy");
}

int nbody_external_at(NbodyHandle* h, const double* xyz, size_t n_points, double* acc, double* phi) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = external_enter(h, "nbody_external_at");
    if (rc) return rc;
    if (n_points > (size_t(1) << 30)) return fail(h, NBODY_ERR_INVALID, "nbody_external_at: n_points must not exceed 2^30");
    if (!xyz && n_points > 0) return fail(h, NBODY_ERR_INVALID, "nbody_external_at: xyz is NULL");
    return nbody::ext::at(h, g_of(h), xyz, n_points, acc, phi);
}

// ---- diagnostics of the state as a whole (nbody_diag.cpp)
namespace {
// binds the device, refuses the handles the diagnostics do not take, naming the entry point, and confirms the steps enqueued
// without a read-back (the readers want the state those steps produced).  The host's view of the body count is NOT refreshed:
// the kernels read the live count on the device.
int diag_enter(NbodyHandle* h, const char* call) {
    int rc = use_device(h);
    if (rc) return rc;
    if (const char* why = nbody::diag::refusal(h)) return fail(h, NBODY_ERR_INVALID, std::string(call) + ": " + why);
    return resolve_async(h);
}
}  // namespace

int nbody_moments(NbodyHandle* h, double out[10]) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_moments");
    if (rc) return rc;
    if (!out) return fail(h, NBODY_ERR_INVALID, "nbody_moments: out is NULL");
    if (h->f64) return nbody::diag::moments(h, nbody64::shard(h), nbody64::n_upper(h), out);
    return nbody::diag::moments(h, h->sh, h->n_local, out);
}

int nbody_lagrangian_radii(NbodyHandle* h, const double center[3], const double* fractions, size_t n_frac, double* radii, double* mass_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_lagrangian_radii");
    if (rc) return rc;
    if (n_frac > (size_t(1) << 20)) return fail(h, NBODY_ERR_INVALID, "nbody_lagrangian_radii: n_frac must not exceed 2^20");
    if (n_frac > 0 && !fractions) return fail(h, NBODY_ERR_INVALID, "nbody_lagrangian_radii: fractions is NULL");
    if (n_frac > 0 && !radii) return fail(h, NBODY_ERR_INVALID, "nbody_lagrangian_radii: radii is NULL");
    for (size_t k = 0; k < n_frac; ++k)
        if (!(fractions[k] >= 0.0 && fractions[k] <= 1.0))   // (a NaN fails both comparisons)
            return fail(h, NBODY_ERR_INVALID, "nbody_lagrangian_radii: fraction " + std::to_string(k) + " is not in [0, 1]");
    if (h->f64) return nbody::diag::lagrangian_radii(h, nbody64::shard(h), nbody64::n_upper(h), center, fractions, n_frac, radii, mass_out);
    return nbody::diag::lagrangian_radii(h, h->sh, h->n_local, center, fractions, n_frac, radii, mass_out);
}

// ---- binary census (nbody_pairs.cpp): the contract of the diagnostics above, diag_enter included
namespace {
void g_and_soft(const NbodyHandle* h, double* g, double* g_soft) {   // the handle's, widened
    *g = double(h->g);
    *g_soft = double(h->g_soft);
    if (h->f64) nbody64::get_settings(h, g, g_soft, nullptr, nullptr);
}
}  // namespace

int nbody_partners(NbodyHandle* h, int32_t* partner, double* energy, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_partners");
    if (rc) return rc;
    double g = 0.0, g_soft = 0.0;
    g_and_soft(h, &g, &g_soft);
    if (h->f64) return nbody::pairs::partners(h, nbody64::shard(h), nbody64::n_upper(h), g, g_soft, partner, energy, cap, n_out);
    return nbody::pairs::partners(h, h->sh, h->n_local, g, g_soft, partner, energy, cap, n_out);
}

int nbody_bound_pairs(NbodyHandle* h, NbodyBoundPair* pairs, size_t cap, size_t* n_pairs, double* binding_sum) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_bound_pairs");
    if (rc) return rc;
    double g = 0.0, g_soft = 0.0;
    g_and_soft(h, &g, &g_soft);
    if (h->f64) return nbody::pairs::bound_pairs(h, nbody64::shard(h), nbody64::n_upper(h), g, g_soft, pairs, cap, n_pairs, binding_sum);
    return nbody::pairs::bound_pairs(h, h->sh, h->n_local, g, g_soft, pairs, cap, n_pairs, binding_sum);
}

// ---- sticky mergers (nbody_pairs.cpp): nearest and contacts under the census's contract; merge_contacts begins like
// nbody_remove_point (diag_enter settles enqueued steps and a poisoned device build) and, when it merged, ends like it
namespace {
int contact_radius(NbodyHandle* h, const char* call, double radius) {
    if (std::isfinite(radius) && radius > 0.0) return NBODY_OK;
    return fail(h, NBODY_ERR_INVALID, std::string(call) + ": radius must be finite and > 0");
}
}  // namespace

int nbody_nearest(NbodyHandle* h, int32_t* nearest, double* dist2, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_nearest");
    if (rc) return rc;
    if (h->f64) return nbody::pairs::nearest(h, nbody64::shard(h), nbody64::n_upper(h), nearest, dist2, cap, n_out);
    return nbody::pairs::nearest(h, h->sh, h->n_local, nearest, dist2, cap, n_out);
}

int nbody_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_contacts");
    if (!rc) rc = contact_radius(h, "nbody_contacts", radius);
    if (rc) return rc;
    if (h->f64) return nbody::pairs::contacts(h, nbody64::shard(h), nbody64::n_upper(h), radius, list, cap, n_contacts);
    return nbody::pairs::contacts(h, h->sh, h->n_local, radius, list, cap, n_contacts);
}

int nbody_merge_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = diag_enter(h, "nbody_merge_contacts");
    if (!rc) rc = contact_radius(h, "nbody_merge_contacts", radius);
    if (rc) return rc;
    if (h->f64) return nbody64::merge_contacts(h, radius, list, cap, n_contacts);
    // (an f32 handle keeps nothing beside the count that a removal makes stale: every force pass builds its tree anew)
    return nbody::pairs::merge_contacts<float>(h, *h, radius, list, cap, n_contacts, nullptr,
                                               [](NbodyHandle* hh, int n_upper) { nbody::launch_compact(hh->stream, hh->sh, n_upper); });
}

// ---- tracers (nbody_tracer.cpp)
namespace {
// binds the device, refuses the handles that take no tracers, naming the entry point, and confirms the steps enqueued without
// a read-back (a poisoned run is replayed first: the tracers ride in those steps, so every reader and the upload come after them,
// like nbody_download, nbody_count, nbody_stats and nbody_upload on the bodies' side)
int tracer_enter(NbodyHandle* h, const char* call) {
    int rc = use_device(h);
    if (rc) return rc;
    if (const char* why = nbody::tracer::refusal(h)) return fail(h, NBODY_ERR_INVALID, std::string(call) + ": " + why);
    return resolve_async(h);
}
}  // namespace

int nbody_tracers_upload(NbodyHandle* h, const void* aos, size_t n, size_t stride, size_t capacity) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = tracer_enter(h, "nbody_tracers_upload");
    if (rc) return rc;
    if (!aos && n) return fail(h, NBODY_ERR_INVALID, "nbody_tracers_upload: null argument");
    if (stride < 40 || stride % 4) return fail(h, NBODY_ERR_INVALID, "nbody_tracers_upload: stride must be a multiple of 4 and >= 40 bytes");
    return nbody::tracer::upload(h, aos, n, stride, capacity);
}

int nbody_tracers_download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = tracer_enter(h, "nbody_tracers_download");
    if (rc) return rc;
    if (stride < 40 || stride % 4) return fail(h, NBODY_ERR_INVALID, "nbody_tracers_download: stride must be a multiple of 4 and >= 40 bytes");
    return nbody::tracer::download(h, aos, cap, stride, n_out);
}

int nbody_tracers_count(NbodyHandle* h, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = tracer_enter(h, "nbody_tracers_count");
    if (rc) return rc;
    if (!n_out) return fail(h, NBODY_ERR_INVALID, "nbody_tracers_count: null argument");
    return nbody::tracer::count(h, n_out);
}

int nbody_tracer_stats(NbodyHandle* h, uint64_t out[2]) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = tracer_enter(h, "nbody_tracer_stats");
    if (rc) return rc;
    if (!out) return fail(h, NBODY_ERR_INVALID, "nbody_tracer_stats: null argument");
    return nbody::tracer::stats(h, out);
}

int nbody_host_tracer_plan(size_t n_tracers, size_t n_bodies, int out[4]) {
    if (!out) return NBODY_ERR_INVALID;
    const nbody::TracerPlan p = nbody::tracer_plan(n_tracers, n_bodies);
    out[0] = p.ipt; out[1] = p.groups; out[2] = p.K; out[3] = p.slice_len;
    return NBODY_OK;
}

int nbody_elapsed(const NbodyHandle* h, float* out) {
    if (!h || !out) return NBODY_ERR_INVALID;
    *out = h->f64 ? float(nbody64::elapsed(h)) : h->elapsed;
    return NBODY_OK;
}

int nbody_elapsed_f64(const NbodyHandle* h, double* out) {
    if (!h || !out) return NBODY_ERR_INVALID;
    *out = h->f64 ? nbody64::elapsed(h) : double(h->elapsed);
    return NBODY_OK;
}

int nbody_sync(NbodyHandle* h) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    rc = resolve_async(h);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return comm_check(h);
}

int nbody_set_profiling(NbodyHandle* h, int on) {
    if (!h) return NBODY_ERR_INVALID;
    h->profiling = on != 0;
    h->profile_every = on > 1 ? on : 1;
    h->profile_tick = 0;
    return NBODY_OK;
}

int nbody_stats(NbodyHandle* h, NbodyStats* out) {
    if (!h || !out) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    rc = resolve_async(h);
    if (rc) return rc;
    rc = drain_events(h);
    if (rc) return rc;
    if (h->f64) return nbody64::stats(h, out);
    if (h->cfg.method == NBODY_BRUTE_FORCE) {
        unsigned long long* hv = reinterpret_cast<unsigned long long*>(h->h_poison + kScratchStats);
        HIP_TRY(h, hipMemcpyAsync(hv, h->sh.inter, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->stats.interactions = *hv;
    }
    if (h->d_counters) {
        HIP_TRY(h, hipMemcpyAsync(h->h_counters, h->d_counters, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        unsigned long long acc_sum = 0, vis_sum = 0;
        for (unsigned k = 0; k < NBODY_WALK_COUNTER_SLOTS; ++k) { acc_sum += h->h_counters[2 * k]; vis_sum += h->h_counters[2 * k + 1]; }
        h->stats.interactions = acc_sum;
        h->stats.force_kernel_interactions = acc_sum;  // the walk kernel evaluates all of them
        h->stats.node_visits = vis_sum;
    }
    *out = h->stats;
    return NBODY_OK;
}

int nbody_reset_stats(NbodyHandle* h) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    rc = resolve_async(h);
    if (rc) return rc;
    rc = drain_events(h);
    if (rc) return rc;
    uint64_t nodes = h->stats.tree_nodes;
    h->stats = NbodyStats{};
    h->stats.tree_nodes = nodes;
    if (h->let) { rc = nbody::let::reset_stats(h); if (rc) return rc; }
    if (h->f64) { rc = nbody64::reset_stats(h); if (rc) return rc; }
    else HIP_TRY(h, hipMemsetAsync(h->sh.inter, 0, sizeof(unsigned long long), h->stream));
    rc = nbody::tracer::reset_stats(h);
    if (rc) return rc;
    if (h->d_counters) {
        HIP_TRY(h, hipMemsetAsync(h->d_counters, 0, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return NBODY_OK;
}

int nbody_energy(NbodyHandle* h, double* kinetic, double* potential) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (h->f64) return nbody64::energy(h, kinetic, potential);
    if (h->let && h->cfg.world_size > 1)   // (a spatial rank sees its own bodies only: the pair sum over them is not the world's energy)
        return fail(h, NBODY_ERR_INVALID, "nbody_energy is not supported on NBODY_SHARD_SPATIAL handles of a world of more than one rank");
    rc = resolve_async(h);
    if (rc) return rc;
    rc = h->sync_count(h, h->stream);
    if (rc) return rc;
    const size_t n = h->n_local;
    const size_t blocks = (n + 255) / 256;
    double ke = 0.0, pe = 0.0;
    if (blocks) {
        HIP_TRY(h, grow_dev(h, h->d_energy, h->energy_blocks, blocks, 2 * sizeof(double), Grow::exact));
        nbody::launch_energy(h->stream, h->sh, int(n), double(h->g_soft) * double(h->g_soft), h->d_energy);
        HIP_TRY(h, hipGetLastError());
        std::vector<double> part(blocks * 2);
        HIP_TRY(h, hipMemcpyAsync(part.data(), h->d_energy, blocks * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t b = 0; b < blocks; ++b) { ke += part[2 * b]; pe += part[2 * b + 1]; }
    }
    if (kinetic) *kinetic = ke;
    if (potential) *potential = -0.5 * double(h->g) * pe;  // every unordered pair was met twice
    return NBODY_OK;
}

int nbody_potentials(NbodyHandle* h, int mode, double* phi, size_t cap, size_t* n_out, uint64_t counts[2]) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    size_t n = 0;
    nbody::PotBodies bodies;
    double g = 0.0;
    rc = potentials_device(h, mode, &n, &bodies, &g);
    if (rc) return rc;
    return nbody::pot::download(h, n, g, phi, cap, n_out, counts);
}

namespace {
// what nbody_field_at and nbody_tidal_at (`who`) share: the checks of the probes and potentials_device(.., field = true)
int probes_begin(NbodyHandle* h, const char* who, int mode, const double* xyz, size_t n_points, nbody::PotBodies* bodies, double* g) {
    if (n_points > (size_t(1) << 30)) return fail(h, NBODY_ERR_INVALID, std::string(who) + ": n_points must not exceed 2^30");
    if (!xyz && n_points > 0) return fail(h, NBODY_ERR_INVALID, std::string(who) + ": xyz is NULL");
    h->field.n_points = n_points;
    h->field.nodes = nullptr; h->field.n_nodes = 0; h->field.K = 1; h->field.quad = nullptr;
    size_t n = 0;
    return potentials_device(h, mode, &n, bodies, g, true);
}
}  // namespace

int nbody_field_at(NbodyHandle* h, int mode, const double* xyz, size_t n_points, double* acc, double* phi, uint64_t counts[2]) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    nbody::PotBodies bodies;
    double g = 0.0;
    rc = probes_begin(h, "nbody_field_at", mode, xyz, n_points, &bodies, &g);
    if (rc) return rc;
    nbody::field::Out out;
    out.acc = acc; out.phi = phi;
    return nbody::field::run(h, mode, bodies, g, xyz, n_points, out, counts);
}

int nbody_tidal_at(NbodyHandle* h, int mode, const double* xyz, size_t n_points, double* tidal6, uint64_t counts[2]) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (mode == NBODY_POTENTIAL_TREE_QUADRUPOLE)
        return fail(h, NBODY_ERR_INVALID, "nbody_tidal_at: NBODY_POTENTIAL_TREE_QUADRUPOLE is not supported (the quadrupole term's share of the tensor is out of scope): NBODY_POTENTIAL_TREE is the tree mode");
    if (h->let)
        return fail(h, NBODY_ERR_INVALID, "nbody_tidal_at is not possible on NBODY_SHARD_SPATIAL handles: a rank holds neither the world's bodies nor the tree around a foreign point");
    nbody::PotBodies bodies;
    double g = 0.0;
    rc = probes_begin(h, "nbody_tidal_at", mode, xyz, n_points, &bodies, &g);
    if (rc) {   // (the preparation's refusals do not know who asked)
        const std::string why = h->err;
        return why.find("nbody_tidal_at") == std::string::npos ? fail(h, rc, "nbody_tidal_at: " + why) : rc;
    }
    nbody::field::Out out;
    out.tidal6 = tidal6; out.tidal = true;
    return nbody::field::run(h, mode, bodies, g, xyz, n_points, out, counts);
}

int nbody_energy_world(NbodyHandle* h, int mode, double* kinetic, double* potential) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    size_t n = 0;
    nbody::PotBodies bodies;
    double g = 0.0;
    rc = potentials_device(h, mode, &n, &bodies, &g);
    if (rc) return rc;
    return nbody::pot::energy(h, bodies, n, g, kinetic, potential);
}

int nbody_tree_export(NbodyHandle* h, float* com_mass, float* width, int32_t* skip, size_t cap, size_t* n_nodes) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->cfg.method != NBODY_BARNES_HUT) return fail(h, NBODY_ERR_INVALID, "not a Barnes-Hut handle");
    if (h->f64) {
        if (com_mass || width) return fail(h, NBODY_ERR_INVALID, "f64 handle: use nbody_tree_export_f64");
        return nbody_tree_export_f64(h, nullptr, nullptr, skip, cap, n_nodes);
    }
    if (h->let)   // (a spatial rank holds its slice and what it imported, never the whole tree)
        return fail(h, NBODY_ERR_INVALID, "nbody_tree_export is not supported on NBODY_SHARD_SPATIAL handles");
    {
        int rc = use_device(h);
        if (rc) return rc;
        rc = resolve_async(h);
        if (rc) return rc;
    }
    return h->tree.export_nodes(h, com_mass, width, skip, cap, n_nodes);
}

namespace {
// why this handle cannot walk with quadrupoles (nullptr: it can)
const char* quadrupole_refusal(const NbodyHandle* h) {
    if (h->cfg.method != NBODY_BARNES_HUT) return "brute-force handles sum every pair exactly: there is no expansion to raise";
    if (h->f64 || h->cfg.dtype != NBODY_F32) return "NBODY_F64 handles walk monopoles only (quadrupoles exist for NBODY_F32)";
    if (h->cfg.math_mode != NBODY_MATH_FAST) return "NBODY_MATH_STRICT reproduces the reference's monopole sums: quadrupoles need NBODY_MATH_FAST";
    if (h->let || h->cfg.shard_mode != NBODY_SHARD_INDEX) return "NBODY_SHARD_SPATIAL handles walk monopoles only";
    if (h->cfg.world_size != 1) return "sharded worlds (world_size > 1) walk monopoles only";
    return nullptr;
}
}  // namespace

int nbody_set_multipole(NbodyHandle* h, int order) {
    if (!h) return NBODY_ERR_INVALID;
    if (order != NBODY_MULTIPOLE_MONOPOLE && order != NBODY_MULTIPOLE_QUADRUPOLE)
        return fail(h, NBODY_ERR_INVALID, "nbody_set_multipole: order must be NBODY_MULTIPOLE_MONOPOLE (1) or NBODY_MULTIPOLE_QUADRUPOLE (2)");
    if (order == NBODY_MULTIPOLE_QUADRUPOLE)
        if (const char* why = quadrupole_refusal(h)) return fail(h, NBODY_ERR_INVALID, std::string("nbody_set_multipole: ") + why);
    if (order != h->multipole && h->async_bh) {   // steps enqueued without read-back are confirmed (or replayed) under the order they were asked with
        int rc = use_device(h);
        if (!rc) rc = resolve_async(h);
        if (rc) return rc;
    }
    h->multipole = order;   // (read by the next force pass)
    return NBODY_OK;
}

int nbody_get_multipole(const NbodyHandle* h, int* order) {
    if (!h || !order) return NBODY_ERR_INVALID;
    *order = h->multipole;
    return NBODY_OK;
}

// ---- nbody_set_integrator: the fourth-order Hermite predictor-corrector of nbody_f64.cpp / kernels_hermite.hip
int nbody_set_integrator(NbodyHandle* h, int integrator) {
    if (!h) return NBODY_ERR_INVALID;
    if (integrator != NBODY_INTEGRATOR_LEAPFROG && integrator != NBODY_INTEGRATOR_HERMITE4)
        return fail(h, NBODY_ERR_INVALID, "nbody_set_integrator: integrator must be NBODY_INTEGRATOR_LEAPFROG (0) or NBODY_INTEGRATOR_HERMITE4 (1)");
    if (integrator == NBODY_INTEGRATOR_HERMITE4) {
        const char* why = h->cfg.method != NBODY_BRUTE_FORCE ? "Barnes-Hut handles step with the leapfrog only"
                        : !h->f64                           ? "NBODY_F32 handles step with the leapfrog only"
                        : h->cfg.world_size != 1            ? "handles of a multi-rank world step with the leapfrog only"
                                                            : nullptr;
        if (why) return fail(h, NBODY_ERR_INVALID, std::string("nbody_set_integrator(NBODY_INTEGRATOR_HERMITE4): ") + why + " (brute-force NBODY_F64 handles with world_size == 1 take it)");
        if (nbody::ext::on(h))
            return fail(h, NBODY_ERR_INVALID, "nbody_set_integrator(NBODY_INTEGRATOR_HERMITE4): an external field is set, and the Hermite step would need its jerk (nbody_set_external_field with n == 0 removes it)");
    }
    if (!h->f64) return NBODY_OK;   // the leapfrog, which is all such a handle runs
    int rc = use_device(h);
    if (rc) return rc;
    return nbody64::set_integrator(h, integrator);
}

int nbody_get_integrator(const NbodyHandle* h, int* integrator) {
    if (!h || !integrator) return NBODY_ERR_INVALID;
    *integrator = h->f64 ? nbody64::get_integrator(h) : NBODY_INTEGRATOR_LEAPFROG;
    return NBODY_OK;
}

int nbody_download_jerk(NbodyHandle* h, double* jerk3, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "nbody_download_jerk: the handle runs the leapfrog integrator (nbody_set_integrator)");
    int rc = use_device(h);
    if (rc) return rc;
    return nbody64::download_jerk(h, jerk3, cap, n_out);
}

int nbody_suggest_dt(NbodyHandle* h, double eta, double* dt_out) {
    if (!h || !dt_out) return h ? fail(h, NBODY_ERR_INVALID, "null argument") : NBODY_ERR_INVALID;
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "nbody_suggest_dt: the handle runs the leapfrog integrator (nbody_set_integrator)");
    int rc = use_device(h);
    if (rc) return rc;
    return nbody64::suggest_dt(h, eta, dt_out);
}

// ---- block individual time steps of a Hermite handle (nbody_f64.cpp hm_block_step): accepted where HERMITE4 is, while it is selected
int nbody_set_block_steps(NbodyHandle* h, double eta, int max_level) {
    if (!h) return NBODY_ERR_INVALID;
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "nbody_set_block_steps: the handle runs the leapfrog integrator (nbody_set_integrator)");
    int rc = use_device(h);
    if (rc) return rc;
    return nbody64::set_block_steps(h, eta, max_level);
}

int nbody_get_block_steps(const NbodyHandle* h, double* eta, int* max_level) {
    if (!h || !h->f64) return NBODY_ERR_INVALID;
    return nbody64::get_block_steps(h, eta, max_level);
}

int nbody_download_levels(NbodyHandle* h, int32_t* level, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "nbody_download_levels: the handle runs the leapfrog integrator (nbody_set_integrator)");
    int rc = use_device(h);
    if (rc) return rc;
    return nbody64::download_levels(h, level, cap, n_out);
}

int nbody_block_step_counts(NbodyHandle* h, uint64_t out[2]) {
    if (!h || !out) return h ? fail(h, NBODY_ERR_INVALID, "null argument") : NBODY_ERR_INVALID;
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "nbody_block_step_counts: the handle runs the leapfrog integrator (nbody_set_integrator)");
    return nbody64::block_step_counts(h, out);
}

int nbody_debug_hermite_forces_of(NbodyHandle* h, const int32_t* ids, size_t n_ids, double* acc3, double* jerk3) {
    if (!h) return NBODY_ERR_INVALID;
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "nbody_debug_hermite_forces_of: the handle runs the leapfrog integrator (nbody_set_integrator)");
    int rc = use_device(h);
    if (rc) return rc;
    return nbody64::debug_hermite_forces_of(h, ids, n_ids, acc3, jerk3);
}

int nbody_tree_export_quadrupoles(NbodyHandle* h, float* q6, size_t cap, size_t* n_nodes) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->cfg.method != NBODY_BARNES_HUT) return fail(h, NBODY_ERR_INVALID, "not a Barnes-Hut handle");
    if (!h->quad_pass && !h->quad_call)
        return fail(h, NBODY_ERR_INVALID, "nbody_tree_export_quadrupoles: neither did the last force pass walk with quadrupoles (nbody_set_multipole) nor was the last tree built by a call in NBODY_POTENTIAL_TREE_QUADRUPOLE");
    int rc = use_device(h);
    if (rc) return rc;
    rc = resolve_async(h);
    if (rc) return rc;
    const size_t n = h->tree.n_nodes;
    if (n_nodes) *n_nodes = n;
    if (!q6) return NBODY_OK;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "tree export buffer too small");
    if (n == 0) return NBODY_OK;
    // of the tree nbody_tree_export reports: the node array as it stands on the device (a tree call of nbody_potentials or
    // nbody_field_at since the force pass has rebuilt it), through the kernel the force pass runs
    HIP_TRY(h, grow_dev(h, h->d_quad, h->quad_cap, std::max(n, h->tree.node_cap), nbody::kQuadRecBytes, Grow::quarter));
    nbody::launch_tree_quad(h->stream, h->tree.d_nodes, int(n), h->d_quad, nullptr, nullptr);
    HIP_TRY(h, hipGetLastError());
    std::vector<float> rec(8 * n);
    HIP_TRY(h, hipMemcpyAsync(rec.data(), h->d_quad, n * nbody::kQuadRecBytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 6; ++k) q6[6 * i + k] = rec[8 * i + k];
    return NBODY_OK;
}

int nbody_tree_export_f64(NbodyHandle* h, double* com_mass, double* width, int32_t* skip, size_t cap, size_t* n_nodes) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->cfg.method != NBODY_BARNES_HUT) return fail(h, NBODY_ERR_INVALID, "not a Barnes-Hut handle");
    if (!h->f64) return fail(h, NBODY_ERR_INVALID, "f32 handle: use nbody_tree_export");
    int rc = use_device(h);
    return rc ? rc : nbody64::tree_export(h, com_mass, width, skip, cap, n_nodes);
}

// ---- the cells of the last tree, for drawing (the reference's Barnes-Hut Renderable walks every node's bounds,
// barnes_hut.rs:322-343).  The node records carry centre of mass, width and skip link, not the box: it is recovered top
// down with the reference's own recurrences -- a node's orthant in its parent is get_orthant(parent centre, its centre
// of mass) (shared.rs:245-254: all its bodies lie in that orthant, so their centre of mass does), its box create_orthant
// (shared.rs:256-272: centre +- half_width / 2, half_width / 2).
extern "C++" {
namespace {
template <class F>
void cells_from_preorder(const F* com_mass, const int32_t* skip, size_t n, const F root_center[3], F root_width, float* min_max6, int32_t* depth) {
    struct Open { size_t end; F c[3]; F half; int depth; };
    std::vector<Open> stack;
    for (size_t i = 0; i < n; ++i) {
        while (!stack.empty() && stack.back().end <= i) stack.pop_back();
        Open me;
        me.end = size_t(skip[i]);
        if (stack.empty()) {
            for (int k = 0; k < 3; ++k) me.c[k] = root_center[k];
            me.half = root_width * F(0.5);     // Bounds::new
            me.depth = 0;
        } else {
            const Open& p = stack.back();
            me.half = p.half * F(0.5);         // create_orthant
            for (int k = 0; k < 3; ++k) me.c[k] = com_mass[4 * i + k] > p.c[k] ? p.c[k] + me.half : p.c[k] - me.half;
            me.depth = p.depth + 1;
        }
        if (min_max6)
            for (int k = 0; k < 3; ++k) {
                min_max6[6 * i + k] = float(me.c[k] + (-me.half));       // Bounds::min (shared.rs:223-225)
                min_max6[6 * i + 3 + k] = float(me.c[k] + me.half);      // Bounds::max
            }
        if (depth) depth[i] = me.depth;
        if (me.end > i + 1) stack.push_back(me);   // it has children: they follow
    }
}
}  // namespace
}  // extern "C++"

int nbody_tree_export_cells(NbodyHandle* h, float* min_max6, int32_t* depth, size_t cap, size_t* n_nodes) {
    if (!h) return NBODY_ERR_INVALID;
    size_t n = 0;
    if (h->f64) {
        int rc = nbody_tree_export_f64(h, nullptr, nullptr, nullptr, 0, &n);
        if (rc) return rc;
        if (n_nodes) *n_nodes = n;
        if (!min_max6 && !depth) return NBODY_OK;
        if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "tree export buffer too small");
        std::vector<double> cm(4 * n), w(n);
        std::vector<int32_t> sk(n);
        rc = nbody_tree_export_f64(h, cm.data(), w.data(), sk.data(), n, &n);
        if (rc) return rc;
        double c[3], width;
        nbody64::get_bounds(h, c, &width);
        cells_from_preorder<double>(cm.data(), sk.data(), n, c, width, min_max6, depth);
        return NBODY_OK;
    }
    int rc = nbody_tree_export(h, nullptr, nullptr, nullptr, 0, &n);
    if (rc) return rc;
    if (n_nodes) *n_nodes = n;
    if (!min_max6 && !depth) return NBODY_OK;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "tree export buffer too small");
    std::vector<float> cm(4 * n), w(n);
    std::vector<int32_t> sk(n);
    rc = nbody_tree_export(h, cm.data(), w.data(), sk.data(), n, &n);
    if (rc) return rc;
    cells_from_preorder<float>(cm.data(), sk.data(), n, h->center, h->width, min_max6, depth);
    return NBODY_OK;
}

int nbody_comm_unique_id(void* id_bytes) {
    if (!id_bytes) return NBODY_ERR_INVALID;
    // NBODY_TRANSPORT=ipc: ranks that share one device (a one-GPU box rehearsing the multi-rank step); default: RCCL
    const char* v = std::getenv("NBODY_TRANSPORT");
    std::string err;
    int rc = nbody::transport_make_id((v && std::strcmp(v, "ipc") == 0) ? nbody::kTransportIpc : nbody::kTransportRccl, id_bytes, &err);
    return rc ? fail(nullptr, rc, err) : NBODY_OK;
}

int nbody_comm_local_id(void* id_bytes) {
    if (!id_bytes) return NBODY_ERR_INVALID;
    std::string err;
    int rc = nbody::transport_make_id(nbody::kTransportIpc, id_bytes, &err);
    return rc ? fail(nullptr, rc, err) : NBODY_OK;
}

// what every rank of a world must agree on: a rank that chose another exchange scheme than its peers would neither send
// nor expect what the others exchange with it (a hang in RCCL), so disagreement is an error at nbody_comm_init
struct Agreement {
    int32_t abi, method, math_mode, leaf_mode, tree_build, dtype, shard_mode, world, seg_cap;
    int32_t cross_sym, sym_packed, bf_variant, walk_variant, walk_split;
    uint64_t capacity;
};
static const char* const kAgreementFields[] = {"ABI version", "method", "math_mode", "leaf_mode", "tree_build", "dtype", "shard_mode", "world_size",
                                               "shard capacity", "NBODY_CROSS_SYM", "NBODY_SYM_PACKED", "NBODY_BF_VARIANT", "NBODY_BH_VARIANT",
                                               "NBODY_BH_SPLIT"};

int nbody_comm_init(NbodyHandle* h, const void* id_bytes) {
    if (!h || !id_bytes) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    h->comm_ready = false;
    h->tp.reset();
    {
        std::string err;
        int code = NBODY_ERR_COMM;
        h->tp.reset(nbody::transport_create(id_bytes, h->cfg.rank, h->cfg.world_size, h->device, &err, &code));
        if (!h->tp) return fail(h, code, err);
    }
    if (!h->comm_stream) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_drifted, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_gathered, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_partials_ready, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_partials_done, hipEventDisableTiming));
    }
    Agreement mine{NBODY_ABI_VERSION, h->cfg.method, h->cfg.math_mode, h->cfg.leaf_mode, h->cfg.tree_build, h->cfg.dtype, h->cfg.shard_mode,
                   h->cfg.world_size, h->sh.seg_cap, nbody::tuning().cross_sym, nbody::tuning().sym_packed, nbody::tuning().bf_fast_variant, nbody::tuning().bh_walk_variant,
                   nbody::tuning().bh_walk_split, h->cfg.capacity};
    std::vector<Agreement> all(size_t(h->cfg.world_size));
    TP_TRY(h, h->tp->host_all_gather(&mine, all.data(), sizeof(Agreement)));
    for (int r = 0; r < h->cfg.world_size; ++r) {
        const int32_t* a = reinterpret_cast<const int32_t*>(&all[size_t(r)]);
        const int32_t* m = reinterpret_cast<const int32_t*>(&mine);
        for (size_t f = 0; f < sizeof(kAgreementFields) / sizeof(kAgreementFields[0]); ++f)
            if (a[f] != m[f]) {
                h->tp.reset();
                return fail(h, NBODY_ERR_COMM, std::string("nbody_comm_init: rank ") + std::to_string(r) + " and rank " + std::to_string(h->cfg.rank) + " disagree on " +
                                                   kAgreementFields[f] + " (" + std::to_string(a[f]) + " vs " + std::to_string(m[f]) + "): every rank of a world must be created alike");
            }
        if (all[size_t(r)].capacity != mine.capacity) {
            h->tp.reset();
            return fail(h, NBODY_ERR_COMM, "nbody_comm_init: ranks disagree on NbodyConfig.capacity");
        }
    }
    h->comm_ready = true;
    return NBODY_OK;
}

// ---- launch-shape and scheme knobs of one handle (kernels.h struct Tuning)
namespace {
struct Knob { const char* name; int nbody::Tuning::*field; bool tuning_build_only; };
const Knob kKnobs[] = {
    {"cross_sym", &nbody::Tuning::cross_sym, false}, {"sym_packed", &nbody::Tuning::sym_packed, false},
    {"bf_fast_variant", &nbody::Tuning::bf_fast_variant, false}, {"sym_wpb", &nbody::Tuning::sym_wpb, false}, {"sym_ipt", &nbody::Tuning::sym_ipt, false}, {"let_list_div", &nbody::Tuning::let_list_div, false}, {"bh_walk_duo", &nbody::Tuning::bh_walk_duo, false}, {"bh_walk_xcd", &nbody::Tuning::bh_walk_xcd, false},
    {"sym_rounds", &nbody::Tuning::sym_rounds, false}, {"sym_k", &nbody::Tuning::sym_k, false},
    {"sym_min_bodies", &nbody::Tuning::sym_min_bodies, false}, {"sym_reduce_split", &nbody::Tuning::sym_reduce_split, false},
    {"sym_opp_rot", &nbody::Tuning::sym_opp_rot, false},
    {"cross_slots", &nbody::Tuning::cross_slots, false}, {"cross_ipt", &nbody::Tuning::cross_ipt, false},
    {"cross_wpb", &nbody::Tuning::cross_wpb, false}, {"bh_walk_split", &nbody::Tuning::bh_walk_split, false},
    {"bh_walk_order", &nbody::Tuning::bh_walk_order, false}, {"bh_reduce_split", &nbody::Tuning::bh_reduce_split, false},
    {"tree_max_tie", &nbody::Tuning::tree_max_tie, false},
    {"bf64_min_bodies", &nbody::Tuning::bf64_min_bodies, false}, {"bf64_ipt", &nbody::Tuning::bf64_ipt, false},
    {"bf64_rot", &nbody::Tuning::bf64_rot, false}, {"bf64_waves", &nbody::Tuning::bf64_waves, false},
    {"bh_walk_variant", &nbody::Tuning::bh_walk_variant, true}, {"bh_walk_lds_block", &nbody::Tuning::bh_walk_lds_block, true},
    {"bh_hot_cap", &nbody::Tuning::bh_hot_cap, true}, {"bh_walk_debug", &nbody::Tuning::bh_walk_debug, true},
    {"sym_debug", &nbody::Tuning::sym_debug, true},
};
}  // namespace

int nbody_set_tuning(NbodyHandle* h, const char* name, int value) {
    if (!h || !name) return NBODY_ERR_INVALID;
    for (const Knob& k : kKnobs)
        if (std::strcmp(k.name, name) == 0) {
#ifndef NBODY_TUNING
            if (k.tuning_build_only && value != nbody::Tuning{}.*(k.field))
                return fail(h, NBODY_ERR_INVALID, std::string("nbody_set_tuning: '") + name + "' selects code only the tuning build carries (make -C nbody-llm_amd/csrc tuning)");
#endif
            if (h->comm_ready && (std::strcmp(name, "cross_sym") == 0 || std::strcmp(name, "sym_packed") == 0 || std::strcmp(name, "bf_fast_variant") == 0))
                return fail(h, NBODY_ERR_INVALID, std::string("nbody_set_tuning: '") + name + "' is part of what the ranks agreed on at nbody_comm_init: set it before");
            h->tune.*(k.field) = value;
            return NBODY_OK;
        }
    return fail(h, NBODY_ERR_INVALID, std::string("nbody_set_tuning: unknown knob '") + name + "'");
}

int nbody_get_tuning(const NbodyHandle* h, const char* name, int* value) {
    if (!h || !name || !value) return NBODY_ERR_INVALID;
    for (const Knob& k : kKnobs)
        if (std::strcmp(k.name, name) == 0) { *value = h->tune.*(k.field); return NBODY_OK; }
    return NBODY_ERR_INVALID;
}

int nbody_get_config(const NbodyHandle* h, NbodyConfig* out) {
    if (!h || !out) return NBODY_ERR_INVALID;
    *out = h->cfg;   // (as created, with tree_build and math_mode resolved at nbody_create)
    return NBODY_OK;
}

int nbody_is_tuning_build(void) {
#ifdef NBODY_TUNING
    return 1;
#else
    return 0;
#endif
}

int nbody_comm_transport(const NbodyHandle* h, char* out, size_t cap) {
    if (!h || !out || cap == 0) return NBODY_ERR_INVALID;
    std::snprintf(out, cap, "%s", h->tp ? h->tp->name() : "none");
    return NBODY_OK;
}

int nbody_download_ids(NbodyHandle* h, int32_t* ids, size_t cap, size_t* n_out) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (!h->let) return fail(h, NBODY_ERR_INVALID, "nbody_download_ids is for NBODY_SHARD_SPATIAL handles (index-block shards: nbody_local_range)");
    return nbody::let::download_ids(h, ids, cap, n_out);
}

int nbody_let_stats(NbodyHandle* h, NbodyLetStats* out) {
    if (!h || !out) return NBODY_ERR_INVALID;
    if (!h->let) return fail(h, NBODY_ERR_INVALID, "not an NBODY_SHARD_SPATIAL handle");
    return nbody::let::stats(h, out);
}

int nbody_debug_let_phase(NbodyHandle* h, int phase, float dt) {
    if (!h) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (!h->let) return fail(h, NBODY_ERR_INVALID, "not an NBODY_SHARD_SPATIAL handle");
    return nbody::let::debug_phase(h, phase, dt);
}

int nbody_debug_let_exchange(NbodyHandle* h, NbodyHandle* peer, int which) {
    if (!h || !peer) return NBODY_ERR_INVALID;
    int rc = use_device(h);
    if (rc) return rc;
    if (!h->let || !peer->let) return fail(h, NBODY_ERR_INVALID, "not an NBODY_SHARD_SPATIAL handle");
    return nbody::let::debug_exchange(h, peer, which);
}

int nbody_debug_let_set_prune(NbodyHandle* h, int prune);   // (nbody_let.cpp owns the state)

int nbody_local_range(const NbodyHandle* h, size_t* first, size_t* count) {
    if (!h) return NBODY_ERR_INVALID;
    if (first) *first = h->first_global;
    if (count) *count = h->n_at_upload;
    return NBODY_OK;
}

// ---- test hooks: a sharded step with the exchange done by the caller --------------------------
// Two handles of one process (ranks 0..G-1 of a world of G, all on the same device) can stand in
// for G GPUs: step_begin on each, import every peer's segment into each, step_end on each.  This
// is what nbody_step_by does around the RCCL all-gather; only the transport differs.
int nbody_debug_step_begin(NbodyHandle* h, float dt) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->f64) return fail(h, NBODY_ERR_INVALID, "f64 handles are single-shard");
    int rc = use_device(h);
    return rc ? rc : step_begin(h, dt);
}

int nbody_debug_import_segment(NbodyHandle* h, NbodyHandle* peer) {
    if (!h || !peer) return NBODY_ERR_INVALID;
    if (h->f64 || peer->f64) return fail(h, NBODY_ERR_INVALID, "f64 handles are single-shard");
    if (h->sh.n_seg != peer->sh.n_seg || h->sh.seg_cap != peer->sh.seg_cap) return fail(h, NBODY_ERR_INVALID, "peer has a different sharding");
    int rc = use_device(h);
    if (rc) return rc;
    const int s = peer->sh.my_seg;
    HIP_TRY(h, hipStreamSynchronize(peer->stream));
    HIP_TRY(h, hipMemcpyAsync(h->sh.pos_all + size_t(s) * h->sh.seg_cap, peer->sh.own_pos(), size_t(h->sh.seg_cap) * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->sh.seg_count + s, peer->sh.own_count(), sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->count_dirty = true;
    return NBODY_OK;
}

int nbody_debug_step_forces(NbodyHandle* h, float dt) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->f64) return fail(h, NBODY_ERR_INVALID, "f64 handles are single-shard");
    int rc = use_device(h);
    return rc ? rc : step_forces(h, dt);
}

// what the grouped ncclSend/ncclRecv round delivers: the partial sums `peer` accumulated for this
// shard's bodies, into the plane reserved for that sender
int nbody_debug_import_partials(NbodyHandle* h, NbodyHandle* peer) {
    if (!h || !peer) return NBODY_ERR_INVALID;
    if (h->f64 || peer->f64) return fail(h, NBODY_ERR_INVALID, "f64 handles are single-shard");
    int rc = use_device(h);
    if (rc) return rc;
    if (!(h->cross_on && h->tail_pending)) return NBODY_OK;   // this force pass exchanges nothing
    if (!(peer->cross_on && peer->tail_pending)) return fail(h, NBODY_ERR_INVALID, "peer is not in the same phase");
    int src = -1, dst = -1;
    for (int i = 0; i < peer->cross.parts.n; ++i) if (peer->cross.parts.seg[i] == h->sh.my_seg) src = i;
    for (int i = 0; i < h->cross.n_recv; ++i) if (h->cross.recv_from[i] == peer->sh.my_seg) dst = i;
    if ((src < 0) != (dst < 0)) return fail(h, NBODY_ERR_INVALID, "send/receive plans of the two shards do not match");
    if (src < 0) return NBODY_OK;
    HIP_TRY(h, hipStreamSynchronize(peer->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_planes + size_t(h->recv_plane0 + dst) * h->sym_plan.plane_stride,
                              peer->d_send + size_t(src) * peer->sym_plan.plane_stride,
                              size_t(h->sh.seg_cap) * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}

int nbody_debug_step_end(NbodyHandle* h, float dt) {
    if (!h) return NBODY_ERR_INVALID;
    if (h->f64) return fail(h, NBODY_ERR_INVALID, "f64 handles are single-shard");
    int rc = use_device(h);
    return rc ? rc : step_finish(h, dt);
}

// Host-only entry (no device needed): which pairs between shards this rank evaluates and whom it
// exchanges partial sums with (kernels_bf_cross.hip make_cross_plan), for tests of the host logic.
// parts: n_parts rows {shard, c0, c1, a0, a1}; recv_from: n_recv ranks in the order their planes are added.
int nbody_host_cross_plan(int rank, int world, int seg_cap, int n_own, int* ipt, int* n_sets, int* n_parts, int* parts,
                          int* n_recv, int* recv_from) {
    if (world < 2 || rank < 0 || rank >= world || seg_cap <= 0 || n_own < 0 || n_own > seg_cap) return NBODY_ERR_INVALID;
    if (world > 2 * (nbody::CrossPartners::kMax - 1)) return NBODY_ERR_INVALID;
    const nbody::CrossPlan p = nbody::make_cross_plan(rank, world, seg_cap, n_own);
    if (ipt) *ipt = p.ipt;
    if (n_sets) *n_sets = p.A;
    if (n_parts) *n_parts = p.parts.n;
    if (parts)
        for (int i = 0; i < p.parts.n; ++i) {
            parts[5 * i + 0] = p.parts.seg[i]; parts[5 * i + 1] = p.parts.c0[i]; parts[5 * i + 2] = p.parts.c1[i];
            parts[5 * i + 3] = p.parts.a0[i]; parts[5 * i + 4] = p.parts.a1[i];
        }
    if (n_recv) *n_recv = p.n_recv;
    if (recv_from) for (int i = 0; i < p.n_recv; ++i) recv_from[i] = p.recv_from[i];
    return NBODY_OK;
}

// Host-only entry (no device needed): the launch shapes the library's defaults give n_bodies -- the Barnes-Hut walk's bodies
// per lane and node-range segments (walk_plan) and the symmetric kernel's bodies per lane -- for tests of the rule.
int nbody_host_launch_plan(size_t n_bodies, float theta2, int fast_math, int out[3]) {
    if (!out) return NBODY_ERR_INVALID;
    nbody::bind_tuning(nullptr);   // (the library's defaults, not some handle's knobs)
    const nbody::WalkPlan p = nbody::walk_plan(n_bodies, fast_math != 0, nbody::kMaxSplit, theta2);
    out[0] = p.bodies_per_lane; out[1] = p.segments; out[2] = nbody::sym_bodies_per_lane(n_bodies);
    return NBODY_OK;
}

// Host-only entry (no device needed): where the variable-size rounds of the spatial step (migrants, tree nodes) put their
// messages, from the all-gathered G x G count matrix -- the arithmetic sender and receiver of every pair share.
int nbody_host_exchange_layout(const int* matrix, int world, int rank, long long clamp, int packed_send, size_t send_stride,
                               size_t* out_at, size_t* n_out, size_t* in_at, size_t* n_in, size_t* total_in) {
    if (!matrix || world < 1 || world > 16 || rank < 0 || rank >= world || !out_at || !n_out || !in_at || !n_in) return NBODY_ERR_INVALID;
    const size_t t = nbody::let::exchange_layout(matrix, world, rank, clamp, packed_send != 0, send_stride, out_at, n_out, in_at, n_in);
    if (total_in) *total_in = t;
    return NBODY_OK;
}

// Host-only entry (no device needed): the octree build alone, for tests of the host logic.
// Arrays hold `cap` nodes (com_mass 4 floats per node); order holds n body ids.
int nbody_host_build_tree(const float* pos4, size_t n, const float center[3], float width, int threads,
                          float* com_mass, float* node_width, int32_t* skip, int32_t* leaf_body, int32_t* order,
                          size_t cap, size_t* n_nodes) {
    if ((!pos4 && n) || !center || !n_nodes) return NBODY_ERR_INVALID;
    if (n > (1ull << 30)) return NBODY_ERR_INVALID;
    // pool, scratch and output arrays persist per calling thread (repeat calls time the build itself)
    static thread_local std::unique_ptr<nbody::WorkerPool> tl_pool;
    static thread_local int tl_threads = 0;
    static thread_local nbody::BuildScratch scratch;
    static thread_local nbody::HostTree tree;
    const int want = threads > 0 ? threads : 1;
    if (!tl_pool || tl_threads != want) { tl_pool.reset(new nbody::WorkerPool(want)); tl_threads = want; }
    nbody::WorkerPool& pool = *tl_pool;
    int cnt = int(n);
    nbody::build_octree(pos4, 1, int(n), &cnt, center, width, pool, scratch, tree);
    if (tree.too_deep) return NBODY_ERR_TREE_DEPTH;
    *n_nodes = tree.n_nodes;
    if (!com_mass) return NBODY_OK;
    if (tree.n_nodes > cap) return NBODY_ERR_CAPACITY;
    for (size_t i = 0; i < tree.n_nodes; ++i) {
        const nbody::NodeRec& r = tree.nodes[i];
        com_mass[4 * i] = r.a.x; com_mass[4 * i + 1] = r.a.y; com_mass[4 * i + 2] = r.a.z; com_mass[4 * i + 3] = r.a.m;
        if (node_width) node_width[i] = std::sqrt(r.b.w2);
        if (skip) skip[i] = r.b.skip;
        if (leaf_body) leaf_body[i] = r.b.body;
    }
    if (order) std::memcpy(order, tree.order, tree.n_order * sizeof(int32_t));
    return NBODY_OK;
}

}  // extern "C"
