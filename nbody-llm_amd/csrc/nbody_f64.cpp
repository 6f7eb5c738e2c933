// nbody_f64.cpp -- host orchestration of an F = f64 handle: the reference's `Simulation<f64, 3, PointParticle<f64,3>, _>`
// (the instantiation its own driver uses, src/main.rs:52-105).  Strict arithmetic with the octree built on the host in f64
// (octree_host.cpp, the same stable 8-way partition as for f32): positions, velocities, accelerations and node counts
// equal the oracle's f64 instantiation bit for bit -- on one shard and over index-block shards alike (the blocks'
// positions and live counts are exchanged once per step through the handle's transport; partners and tree bodies keep
// their global order).  NBODY_MATH_FAST: the fast walk (one running sum per lane, split node range), device build on one
// shard; brute force every unordered pair once (kernels_bf64.hip), the other blocks' bodies one-sided.  Bodies cross the
// boundary as 80-byte records.
#include "nbody_engine.h"
#include "kernels_f64.h"
#include "kernels_hermite.h"
#include "nbody_external.h"
#include "nbody_mesh.h"
#include "nbody_pairs.h"
#include "nbody_pot.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace nbody64 {

// What a fast all-pairs plane pass keeps between calls: kernels_bf64.hip's plan, re-made when its key (the body counts and
// the knobs) changes, the unordered pairs its symmetric kernel meets, and the partial-sum planes (grow only) -- `kinds` planes
// of double4[n_pad] per plane of the plan: 1, the accelerations; 2, the jerks after them (kernels_hermite.h).  ipt_of: the
// bodies per lane the pass's kernels take for a bf64_ipt knob (nullptr: make_bf64_plan's own choice).
struct PlanePass {
    const int kinds;
    int (*const ipt_of)(int bf64_ipt);
    Bf64Plan plan;
    long long key[6] = {-1, -1, -1, -1, -1, -1};
    uint64_t sym_pairs = 0;
    double4* d_planes = nullptr;
    size_t cap = 0;   // double4 entries
    int ensure(NbodyHandle* h, size_t n_local, size_t n_remote, int n_seg);
};

struct State : EngineBodies<double> {   // (the bodies, their host view, the settings and the tree: nbody_handle.h)
    const double* kick_dt = nullptr;   // inside a step: the dt the force pass may apply itself (fast walk, split node range)
    int kicked = 0;
    PlanePass bf{1, nullptr};          // fast brute force (NBODY_MATH_FAST): one kind of planes
    // nbody_set_integrator(NBODY_INTEGRATOR_HERMITE4): the held jerk, the predicted state and the pair-jerk planes
    // (kernels_hermite.h); acc holds the held a0.  hm_valid: (acc, jerk) are F at the current (pos, vel)
    int integrator = NBODY_INTEGRATOR_LEAPFROG;
    bool hm_valid = false;
    HermiteDev hm;
    PlanePass hmp{2, hermite_ipt};     // the pair-jerk pass: two kinds
    // nbody_set_block_steps: block individual time steps of a Hermite handle (off: blk_L == 0).  lv_valid: blk.level holds
    // levels assigned for a macro step of |dt| == lv_dt from derivatives that are still the held ones (needs hm_valid too)
    double blk_eta = 0.0;
    int blk_L = 0;
    bool lv_valid = false;
    double lv_dt = 0.0;
    BlockDev blk;
    int* h_sched = nullptr;       // pinned [2]: {tau*, due bodies} of the block step
    uint64_t blk_steps = 0, blk_updates = 0;   // since nbody_reset_stats
};

// The plan and the planes for this many own and remote bodies under the current knobs (make_bf64_plan's arguments).  A failed
// allocation leaves no plan behind (the next pass tries again); the key is set only once the planes exist for this plan.
int PlanePass::ensure(NbodyHandle* h, size_t n_local, size_t n_remote, int n_seg) {
    const nbody::Tuning& t = nbody::tuning();
    const long long want[6] = {(long long)n_local, (long long)n_remote, t.bf64_min_bodies, t.bf64_ipt, t.bf64_rot, t.bf64_waves};
    if (std::equal(want, want + 6, key)) return NBODY_OK;
    const Bf64Plan made = make_bf64_plan(int(n_local), int(std::min<size_t>(n_remote, 0x7fffffff)), n_seg, ipt_of ? ipt_of(t.bf64_ipt) : 0);
    const size_t need = size_t(kinds) * size_t(made.n_planes) * made.n_pad;
    if (need > cap) std::fill(key, key + 6, -1LL);
    HIP_TRY(h, grow_dev(h, d_planes, cap, need, sizeof(double4), Grow::exact));
    plan = made;
    sym_pairs = bf64_sym_pairs(made, n_local);
    std::copy(want, want + 6, key);
    return NBODY_OK;
}

namespace {

// The own pairs of a plane pass, `sym` then `own` (launchers of the pass's kernels): every pair once by the symmetric kernel
// + the left-over pairs one-sided or, without a symmetric part (no plan for one, or one or two resident sets: the left-over
// pairs are all of them), every pair one-sided.  The HIP events bracket the dominant launch; returns its directed interactions.
template <class Sym, class Own>
uint64_t launch_own_pairs(NbodyHandle* h, const PlanePass& pp, size_t n_local, Sym sym, Own own) {
    if (pp.plan.sym && pp.plan.sym_sets > 0) {
        {
            ForceTimer t(h);
            sym();
        }
        own();
        return 2 * pp.sym_pairs;
    }
    ForceTimer t(h);
    own();
    return uint64_t(n_local) * uint64_t(n_local - 1);
}

// NBODY_MATH_FAST: every own pair once (k_bf64_sym + the left-over pairs one-sided) or, below Tuning::bf64_min_bodies,
// every own pair one-sided; the other blocks' bodies one-sided from the gathered positions; then the planes in a fixed
// order, with the step's kick when there is one.  Enqueues only (no host synchronisation unless the planes grow).
int bf_forces_fast(NbodyHandle* h, State& s, double eps2) {
    if (s.n_local == 0) return NBODY_OK;
    const size_t tot = engine::total_upper(s);
    const size_t n_remote = tot - std::min<size_t>(tot, size_t(s.seg_count_host[size_t(s.sh.my_seg)]));
    int rc = s.bf.ensure(h, s.n_local, n_remote, s.sh.n_seg);
    if (rc) return rc;
    const Bf64Plan& p = s.bf.plan;
    double4* planes = s.bf.d_planes;
    const uint64_t timed = launch_own_pairs(h, s.bf, s.n_local, [&] { launch_bf64_sym(h->stream, s.sh, p, planes, eps2); },
                                            [&] { launch_bf64_own(h->stream, s.sh, p, planes, eps2); });
    const bool timed_this = h->timed_this;
    launch_bf64_remote(h->stream, s.sh, p, planes, eps2);
    launch_bf64_reduce(h->stream, s.sh, p, planes, int(s.n_local), s.g, s.kick_dt);
    if (s.kick_dt) s.kicked = 1;
    HIP_TRY(h, hipGetLastError());
    if (timed_this) h->stats.force_kernel_interactions += timed;
    return NBODY_OK;
}

// ---- the fourth-order Hermite step (kernels_hermite.hip)
int ensure_hermite(NbodyHandle* h, State& s) {
    if (s.hm.jerk) return NBODY_OK;
    const size_t cap = size_t(s.sh.seg_cap);
    double4** arr[] = {&s.hm.jerk, &s.hm.xp, &s.hm.vp, &s.hm.a1, &s.hm.j1};
    for (double4** a : arr) {
        HIP_TRY(h, h->mem.dev(*a, cap * sizeof(double4)));
        HIP_TRY(h, hipMemsetAsync(*a, 0, cap * sizeof(double4), h->stream));
    }
    HIP_TRY(h, h->mem.dev(s.hm.ratio, ((cap + 255) / 256) * sizeof(double)));
    return NBODY_OK;
}

// (a, j) = F(x, v).  c == nullptr: into (out_a, out_j); else the corrector follows (in place on pos / vel / acc / jerk, with
// the retain's flags): a kernel of its own in strict math, inside the plane reduce in fast math.  Enqueues only.
int hm_eval(NbodyHandle* h, State& s, const double4* x, const double4* v, double4* out_a, double4* out_j, const HermiteCoef* c) {
    if (s.n_local == 0) return NBODY_OK;
    const double eps2 = s.g_soft * s.g_soft;
    if (h->cfg.math_mode != NBODY_MATH_FAST) {
        {
            ForceTimer t(h);
            launch_hm_strict(h->stream, s.sh, x, v, c ? s.hm.a1 : out_a, c ? s.hm.j1 : out_j, int(s.n_local), s.g, eps2);
        }
        if (h->timed_this) h->stats.force_kernel_interactions += uint64_t(s.n_local) * uint64_t(s.n_local - 1);
        if (c) launch_hm_correct(h->stream, s.sh, s.hm, int(s.n_local), *c, s.bnd);
        HIP_TRY(h, hipGetLastError());
        return NBODY_OK;
    }
    int rc = s.hmp.ensure(h, s.n_local, 0, 1);   // (one rank: nobody remote)
    if (rc) return rc;
    const Bf64Plan& p = s.hmp.plan;
    double4* planes = s.hmp.d_planes;
    const uint64_t timed = launch_own_pairs(h, s.hmp, s.n_local, [&] { launch_hm_sym(h->stream, s.sh, p, x, v, planes, eps2); },
                                            [&] { launch_hm_own(h->stream, s.sh, p, x, v, planes, eps2); });
    if (h->timed_this) h->stats.force_kernel_interactions += timed;
    launch_hm_reduce(h->stream, s.sh, s.hm, p, planes, int(s.n_local), s.g, out_a, out_j, c, s.bnd);
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

int hm_refresh(NbodyHandle* h, State& s) {   // the held (a0, j0) at the current (x, v)
    int rc = hm_eval(h, s, s.sh.own_pos(), s.sh.vel, s.sh.acc, s.hm.jerk, nullptr);
    if (!rc) s.hm_valid = true;
    s.lv_valid = false;   // (levels belong to the derivatives they were drawn from)
    return rc;
}

// ---- block individual time steps (kernels_hermite.hip, "block individual time steps")
int ensure_block(NbodyHandle* h, State& s) {
    BlockDev& b = s.blk;
    const size_t cap = size_t(s.sh.seg_cap);
    if (!b.level) {
        int** arr[] = {&b.level, &b.tau, &b.list};
        for (int** a : arr) {
            HIP_TRY(h, h->mem.dev(*a, cap * sizeof(int)));
            HIP_TRY(h, hipMemsetAsync(*a, 0, cap * sizeof(int), h->stream));
        }
        HIP_TRY(h, h->mem.dev(b.tile_count, ((cap + 1023) / 1024) * sizeof(int)));
        HIP_TRY(h, h->mem.dev(b.smin, 4 * sizeof(int)));
        HIP_TRY(h, hipMemsetAsync(b.smin, 0, 4 * sizeof(int), h->stream));
        b.sched = b.smin + 2;
        HIP_TRY(h, h->mem.pin(s.h_sched, 2 * sizeof(int)));
    }
    const size_t rows = hm_act_plane_rows(s.sh.seg_cap);   // (follows the bf64_waves knob)
    HIP_TRY(h, grow_dev(h, b.planes, b.plane_rows, rows, 2 * sizeof(double4), Grow::exact));   // accelerations, then jerks
    return NBODY_OK;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// start levels for macro steps of |dt| = abs_dt from the held (valid) derivatives
int assign_levels(NbodyHandle* h, State& s, double abs_dt) {
    int rc = ensure_block(h, s);
    if (rc) return rc;
    launch_hmb_start_levels(h->stream, s.sh, s.hm, s.blk, int(s.n_local), s.blk_eta, abs_dt, s.blk_L);
    HIP_TRY(h, hipGetLastError());
    s.lv_valid = true;
    s.lv_dt = abs_dt;
    return NBODY_OK;
}

// F of the bodies bd.list names (their number is on the device in bd.sched[1] and here in n_act) against all n of (x, v),
// through the active-set kernels of the handle's math mode.  Fast math: into the planes (*plan says how); strict: rows of
// (hm.a1, hm.j1).  Enqueues only.
int hm_act_eval(NbodyHandle* h, State& s, const double4* x, const double4* v, int n_act, HmActPlan* plan) {
    const double eps2 = s.g_soft * s.g_soft;
    if (h->cfg.math_mode == NBODY_MATH_FAST) {
        *plan = make_hm_act_plan(n_act, int(s.n_local));
        if (size_t(plan->K) * size_t(plan->groups) * 64 > s.blk.plane_rows) return fail(h, NBODY_ERR_CAPACITY, "block steps: the active-set planes are too small for this launch");
        launch_hm_act(h->stream, s.sh, s.blk, *plan, x, v, eps2);
    } else {
        launch_hm_act_strict(h->stream, s.sh, s.hm, s.blk, n_act, x, v, s.g, eps2);
    }
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

// One nbody_step_by(dt) of a handle with block steps on: a macro step of T = 2^L ticks (include/nbody_hip.h "block steps").
// The host reads {tau*, due bodies} back once per block step and sizes the force launch from them.
int hm_block_step(NbodyHandle* h, State& s, double dt) {
    if (!s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    int rc = s.sync_count(h, h->stream);   // the exact body count: nothing leaves inside a macro step
    if (!rc && !s.hm_valid) rc = hm_refresh(h, s);
    if (!rc) rc = ensure_block(h, s);
    if (rc) return rc;
    const double abs_dt = std::fabs(dt);
    if (!s.lv_valid || !same_bits(abs_dt, s.lv_dt)) {
        rc = assign_levels(h, s, abs_dt);
        if (rc) return rc;
    }
    const int n = int(s.n_local);
    const int L = s.blk_L, T = 1 << L;
    const double tick = std::ldexp(dt, -L);
    const bool fast = h->cfg.math_mode == NBODY_MATH_FAST;
    if (n > 0) {
        HIP_TRY(h, hipMemsetAsync(s.blk.tau, 0, size_t(n) * sizeof(int), h->stream));
        HIP_TRY(h, hipMemsetAsync(s.blk.smin, 0x7f, 2 * sizeof(int), h->stream));
        for (int k = 0;; ++k) {
            launch_hmb_schedule(h->stream, s.sh, s.hm, s.blk, n, T, tick, k & 1);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(s.h_sched, s.blk.sched, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            const int tstar = s.h_sched[0], n_act = s.h_sched[1];
            if (tstar <= 0 || tstar > T || n_act <= 0 || n_act > n || k >= T)
                return fail(h, NBODY_ERR_HIP, "block steps: the schedule kernels reported an impossible block step");
            HmActPlan plan;
            {
                ForceTimer t(h);
                rc = hm_act_eval(h, s, s.hm.xp, s.hm.vp, n_act, &plan);
            }
            if (rc) return rc;
            if (h->timed_this) h->stats.force_kernel_interactions += uint64_t(n_act) * uint64_t(n - 1);
            launch_hmb_finish(h->stream, s.sh, s.hm, s.blk, fast ? &plan : nullptr, n_act, s.g, T, L, tick, abs_dt, s.blk_eta, s.bnd);
            HIP_TRY(h, hipGetLastError());
            s.blk_steps += 1;
            s.blk_updates += uint64_t(n_act);
            if (tstar == T) break;   // commensurate steps: every body is due at T
        }
        launch_hm_compact(h->stream, s.sh, s.hm, n, s.blk.level);   // retain, on the corrected positions; the levels travel along
        s.count_dirty = true;
        HIP_TRY(h, hipGetLastError());
    }
    s.elapsed += dt;
    h->stats.steps += 1;
    return NBODY_OK;
}

int hm_step(NbodyHandle* h, State& s, double dt) {
    if (s.blk_L > 0 && dt != 0.0) return hm_block_step(h, s, dt);
    if (!s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    int rc = s.hm_valid ? NBODY_OK : hm_refresh(h, s);
    if (rc) return rc;
    const HermiteCoef c = hermite_coef(dt);
    launch_hm_predict(h->stream, s.sh, s.hm, int(s.n_local), c);
    rc = hm_eval(h, s, s.hm.xp, s.hm.vp, nullptr, nullptr, &c);   // + corrector
    if (rc) return rc;
    launch_hm_compact(h->stream, s.sh, s.hm, int(s.n_local));     // retain, on the corrected positions
    s.count_dirty = true;
    s.lv_valid = false;   // (a shared step does not carry block-step levels)
    HIP_TRY(h, hipGetLastError());
    s.elapsed += dt;
    h->stats.steps += 1;
    return NBODY_OK;
}

int bf_forces(NbodyHandle* h, State& s) {
    const double eps2 = s.g_soft * s.g_soft;  // brute_force.rs:69
    if (h->cfg.math_mode == NBODY_MATH_FAST) return bf_forces_fast(h, s, eps2);
    {
        ForceTimer t(h);
        launch_bf_strict(h->stream, s.sh, int(s.n_local), s.g, eps2);
    }
    HIP_TRY(h, hipGetLastError());
    if (h->timed_this && s.n_local > 0) h->stats.force_kernel_interactions += uint64_t(s.n_local) * (uint64_t(engine::total_upper(s)) - 1);
    return NBODY_OK;
}

// The fast walk (NBODY_MATH_FAST on an f64 handle): one running sum per lane, node range split over K segments so that a
// few ten thousand bodies still fill the chip.  `host_nodes` != nullptr: the split points' ancestors are listed here from
// the host-built tree; nullptr: by k_tree_split_anc from the device build's arrays (n_tree bodies).
int fast_walk(NbodyHandle* h, State& s, const Node64* nodes, int n_nodes, const int* order, int n_order, const nbody::NodeRecT<double>* host_nodes, int n_tree,
              int k_done = 0 /* > 0: the split points of this many segments are on the device already (they rode in the build) */) {
    const bool field = h->pot.walking == kWalkField;   // nbody_field_at(TREE): the walk is over the call's probes, not the bodies
    if ((n_order == 0 && !field) || n_nodes <= 0) return NBODY_OK;
    const nbody::WalkPlan plan = walk_split_plan(size_t(n_order), true, float(s.theta2), size_t(n_nodes));   // (bodies per lane x segments: kernels.h)
    const int K = field ? field_split_plan(h->field.n_points, size_t(n_nodes)) : k_done > 0 ? k_done : plan.segments;
    int rc = s.tree.split.ensure(h, K, size_t(s.sh.seg_cap));
    if (!rc && !k_done && host_nodes) rc = s.tree.split.list_on_host(h, h->stream, host_nodes, n_nodes, K);
    if (rc) return rc;
    if (!k_done && !host_nodes) s.tree.split.list_on_device(h->stream, s.tree.work, n_tree, n_nodes, K);
    const WalkSplit64 sp = walk_split_view(s.tree.split, K, size_t(s.sh.seg_cap));
    if (field) {   // the caller walks this tree for its probes, batch by batch (nbody_field.cpp)
        FieldBufs& f = h->field;
        f.nodes = nodes; f.n_nodes = n_nodes; f.K = K;
        f.first = sp.first; f.anc = sp.anc; f.n_anc = sp.n_anc;
        return NBODY_OK;
    }
    if (h->pot.walking) {   // nbody_potentials(NBODY_POTENTIAL_TREE): the same tree, order and split points, walked for potentials
        const size_t stride = (size_t(n_order) + 63) / 64 * 64;
        rc = nbody::pot::ensure_planes(h, size_t(K) * stride);
        if (rc) return rc;
        launch_bh_pot_walk(h->stream, s.sh.own_pos(), nodes, order, n_order, s.g_soft * s.g_soft, s.theta2, sp, h->pot.d_planes, stride, h->pot.d_counts);
        nbody::launch_pot_reduce(h->stream, h->pot.d_planes, K, stride, order, n_order, h->pot.d_sum);
        HIP_TRY(h, hipGetLastError());
        return NBODY_OK;
    }
    {
        ForceTimer t(h);
        launch_bh_walk_fast(h->stream, s.sh, nodes, n_nodes, order, n_order, s.g, s.g_soft * s.g_soft, s.theta2, h->d_counters,
                            h->cfg.leaf_mode == NBODY_LEAF_DIRECT ? 1 : 0, sp, std::min(3, plan.bodies_per_lane), s.kick_dt, &s.kicked);   // (64-byte records, doubles in registers: beyond three per lane the f64 walk loses again -- tools/f64_walk_probe.py)
    }
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

// the reference's nested sums over the tree just built (strict math): one walk per body, `levels` deep at most
int strict_walk(NbodyHandle* h, State& s, const TreeBuilt& t, int levels) {
    const bool direct = h->cfg.leaf_mode == NBODY_LEAF_DIRECT;
    if (!direct) { int rc = s.tree.ensure_stack(h, s.sh.seg_cap, levels); if (rc) return rc; }
    {
        ForceTimer timer(h);
        launch_bh_walk(h->stream, s.sh, s.tree.d_nodes, t.n_nodes, t.order, int(t.n_order), s.g, s.g_soft * s.g_soft, s.theta2, h->d_counters,
                       direct ? 1 : 0, s.tree.d_stack, s.tree.stack_lanes);
    }
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

// The tree built on the device (NBODY_TREE_DEVICE; kernels_tree.hip for double): no positions to the host, no nodes
// back.  Same cells, pre-order and skip links as the host build; centres of mass from double-double prefix sums instead of the
// reference's sequential f64 folds (within 4 units of 2^-53 of the exact centre, cell by cell: tests/tree_moments.py).  *fell_back: coincident bodies / > 42 levels -> the caller builds on the host.
int bh_forces_device(NbodyHandle* h, State& s, bool* fell_back) {
    // one shard, fast math: the walk's split points ride in the build's last launch (kernels.h TreeSplitReq)
    nbody::TreeSplitReq req;
    int k_pre = 0;
    if (s.sh.n_seg == 1 && h->cfg.math_mode == NBODY_MATH_FAST && s.n_local > 0 && h->pot.walking != kWalkField) {   // (a field call draws K from its probes)
        k_pre = walk_split_plan(s.n_local, true, float(s.theta2), s.n_local).segments;   // (a tree has at least as many nodes as bodies)
        int rc = s.tree.bufs.ensure(h, size_t(s.sh.seg_cap), 0);   // (the request names the build's info words)
        if (!rc) rc = s.tree.split.ensure(h, k_pre, size_t(s.sh.seg_cap));
        if (rc) return rc;
        req = s.tree.split.request(k_pre, s.tree.bufs.d_info, nullptr);
    }
    TreeBuilt t;
    int rc = s.tree.build_on_device(h, s, false, k_pre ? &req : nullptr, &t);
    *fell_back = t.fell_back;
    if (rc || t.fell_back) return rc;
    if (h->cfg.math_mode == NBODY_MATH_FAST || h->pot.walking) return fast_walk(h, s, s.tree.d_nodes, t.n_nodes, t.order, int(t.n_order), nullptr, int(t.n_tree), k_pre);
    return strict_walk(h, s, t, 45);   // (the device build goes to 42 levels)
}

// BarnesHutSimulation::update_forces (barnes_hut.rs:250-263): rebuild the tree (host, f64), one walk per body
int bh_forces(NbodyHandle* h, State& s) {
    if (h->cfg.tree_build == NBODY_TREE_DEVICE && (s.sh.n_seg == 1 || h->cfg.math_mode == NBODY_MATH_FAST)) {   // (a sharded world: fast math only, create says so)
        bool fell_back = false;
        int rc = bh_forces_device(h, s, &fell_back);
        if (rc || !fell_back) return rc;
    }
    TreeBuilt t;
    int rc = s.tree.build_on_host(h, s, &t);
    if (rc) return rc;
    if (h->cfg.math_mode == NBODY_MATH_FAST || h->pot.walking)   // (the potential walk runs over the split in strict math too)
        return fast_walk(h, s, s.tree.d_nodes, t.n_nodes, t.order, int(t.n_order), s.tree.host.nodes, int(t.n_tree));
    return strict_walk(h, s, t, s.tree.host.max_depth + 2);   // the tree's depth
}

// mesh gravity: the pass is the mesh field, with the step's kick when there is one; no pair kernel runs
int mesh_forces(NbodyHandle* h, State& s) {
    const int rc = nbody::mesh::pass<double>(h, s.sh, s.n_local, s.g, s.kick_dt, nullptr);
    if (!rc && s.kick_dt) s.kicked = 1;
    return rc;
}

int forces(NbodyHandle* h, State& s) {
    if (nbody::mesh::on(h)) return mesh_forces(h, s);
    return h->cfg.method == NBODY_BARNES_HUT ? bh_forces(h, s) : bf_forces(h, s);
}

// index-block shards: the once-per-step exchange, in place, on the handle's stream
int exchange(NbodyHandle* h, State& s) {
    if (s.sh.n_seg == 1 && !h->comm_ready) return NBODY_OK;
    return engine::gather_blocks(h, s, h->stream);
}

int step_impl(NbodyHandle* h, State& s, double dt) {
    if (s.integrator == NBODY_INTEGRATOR_HERMITE4) return hm_step(h, s, dt);
    if (!s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    launch_drift_half(h->stream, s.sh, int(s.n_local), dt, s.bnd);   // integrate_pre_force
    launch_compact(h->stream, s.sh, int(s.n_local));                 // retain
    s.count_dirty = true;
    HIP_TRY(h, hipGetLastError());
    int rc = exchange(h, s);                                        // sharded: every block's positions and live count
    if (rc) return rc;
    const bool ext = nbody::ext::on(h);                             // an external field: the pass runs as update_forces does, then
    s.kick_dt = ext ? nullptr : &dt; s.kicked = 0;                  // acc += s(x) with the kick (else the fast walk's plane reduction can take the kick along)
    rc = forces(h, s);                                              // update_forces
    s.kick_dt = nullptr;
    if (rc) return rc;
    if (ext) { rc = nbody::ext::add(h, s.sh, s.n_local, s.g, &dt, false); if (rc) return rc; }
    else if (!s.kicked) launch_kick_drift(h->stream, s.sh, int(s.n_local), dt);   // integrate_after_force
    HIP_TRY(h, hipGetLastError());
    s.elapsed += dt;                                                // elapsed += dt
    h->stats.steps += 1;
    return NBODY_OK;
}

}  // namespace

EngineBodies<double>& bodies(NbodyHandle* h) { return *h->f64; }
const EngineBodies<double>& bodies(const NbodyHandle* h) { return *h->f64; }

int create(NbodyHandle* h) {
    State* sp = new State();
    h->f64 = sp;
    State& s = *sp;
    int rc = s.alloc(h, h->stream, h->shape);
    if (rc) return rc;
    if (h->cfg.method == NBODY_BARNES_HUT) { rc = s.tree.alloc_host(h, s.sh); if (rc) return rc; }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}

void destroy(NbodyHandle* h) {
    State* s = h->f64;
    if (!s) return;
    delete s;   // (its device and pinned blocks are the handle's registry's)
    h->f64 = nullptr;
}

int clone_state(NbodyHandle* src, NbodyHandle* dst) {
    State& a = *src->f64;
    State& b = *dst->f64;
    int rc = a.sync_count(src, src->stream);
    if (rc) return rc;
    const size_t cap = size_t(a.sh.seg_cap);
    HIP_TRY(dst, hipStreamSynchronize(src->stream));
    rc = b.copy_from(dst, dst->stream, a);
    if (rc) return rc;
    if (a.integrator == NBODY_INTEGRATOR_HERMITE4) {   // + the held jerk and whether it is valid: the clone steps like its source
        rc = ensure_hermite(dst, b);
        if (rc) return rc;
        HIP_TRY(dst, hipMemcpyAsync(b.hm.jerk, a.hm.jerk, cap * sizeof(double4), hipMemcpyDeviceToDevice, dst->stream));
        b.integrator = a.integrator;
        b.hm_valid = a.hm_valid;
        b.blk_eta = a.blk_eta; b.blk_L = a.blk_L;   // + the block-step setting, the levels and whether they are valid
        if (a.blk_L > 0 && a.lv_valid) {
            rc = ensure_block(dst, b);
            if (rc) return rc;
            HIP_TRY(dst, hipMemcpyAsync(b.blk.level, a.blk.level, cap * sizeof(int), hipMemcpyDeviceToDevice, dst->stream));
            b.lv_valid = true;
            b.lv_dt = a.lv_dt;
        }
    }
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    dst->search.mode = src->search.mode;   // (the clone's statistics start at zero)
    return NBODY_OK;
}

int upload(NbodyHandle* h, const void* aos, size_t n, size_t stride) {
    h->f64->hm_valid = false;
    return engine::upload(h, *h->f64, aos, n, stride);
}

int download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out) {
    return h->f64->download_own(h, h->stream, aos, cap, stride, n_out, nullptr);
}

int count(NbodyHandle* h, size_t* n_out) { return engine::count(h, *h->f64, n_out); }

int count_global(NbodyHandle* h, size_t* n_out) {
    h->f64->count_dirty = true;   // (the exchange wrote the other blocks' counts behind the host's back)
    return engine::count_global(h, *h->f64, n_out);
}

namespace {
// what nbody_remove_point and a merging nbody_merge_contacts leave stale beside the count: the held (a0, j0), and with them the
// block-step levels
void removed(State& s) { s.hm_valid = false; }
}  // namespace

int add_point(NbodyHandle* h, const void* particle) {
    State& s = *h->f64;
    if (s.sh.n_seg > 1) return fail(h, NBODY_ERR_INVALID, "add_point on a sharded f64 world is not supported (f32 handles: collective push / swap_remove)");
    int rc = s.push_one(h, h->stream, particle);
    if (!rc) s.hm_valid = false;
    return rc;
}

int remove_point(NbodyHandle* h, size_t index) {
    State& s = *h->f64;
    if (s.sh.n_seg > 1) return fail(h, NBODY_ERR_INVALID, "remove_point on a sharded f64 world is not supported (f32 handles: collective push / swap_remove)");
    int rc = s.swap_remove_one(h, h->stream, index);
    if (!rc) removed(s);
    return rc;
}

// nbody_merge_contacts: the retain of the handle's integrator (a Hermite handle's carries the jerk and, with block steps on,
// the levels), then what a removal leaves behind
int merge_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts) {
    State& s = *h->f64;
    const bool hermite = s.integrator == NBODY_INTEGRATOR_HERMITE4;
    size_t n = 0;
    int rc = nbody::pairs::merge_contacts<double>(h, s, radius, list, cap, &n, hermite ? s.hm.jerk : nullptr, [](NbodyHandle* hh, int n_upper) {
        State& st = *hh->f64;
        if (st.integrator == NBODY_INTEGRATOR_HERMITE4) launch_hm_compact(hh->stream, st.sh, st.hm, n_upper, st.blk_L > 0 ? st.blk.level : nullptr);
        else nbody::launch_compact(hh->stream, st.sh, n_upper);
    });
    if (n_contacts) *n_contacts = n;
    if (!rc && n) removed(s);
    return rc;
}

int set_settings(NbodyHandle* h, double g, double g_soft, double dt, double theta2) {
    h->f64->set_settings(g, g_soft, dt, theta2);
    h->f64->hm_valid = false;
    return NBODY_OK;
}

int set_bounds(NbodyHandle* h, const double center[3], double width) {
    h->f64->set_bounds(center, width);
    return NBODY_OK;
}

int init(NbodyHandle* h) {
    h->f64->elapsed = 0.0;
    h->f64->hm_valid = false;
    return NBODY_OK;
}

int step_by(NbodyHandle* h, double dt) { return step_impl(h, *h->f64, dt); }

int steps(NbodyHandle* h, int k) {
    State& s = *h->f64;
    for (int i = 0; i < k; ++i) {
        int rc = step_impl(h, s, s.dt);  // Simulation::step, shared.rs:86-88
        if (rc) return rc;
    }
    return NBODY_OK;
}

int update_forces(NbodyHandle* h) {
    State& s = *h->f64;
    if (h->cfg.method == NBODY_BARNES_HUT && !s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    if (s.integrator == NBODY_INTEGRATOR_HERMITE4) {
        int rc = hm_refresh(h, s);
        if (!rc && s.blk_L > 0) {   // + start levels for a macro step of the settings' dt
            rc = s.sync_count(h, h->stream);
            if (!rc) rc = assign_levels(h, s, std::fabs(s.dt));
        }
        return rc;
    }
    int rc = exchange(h, s);
    if (rc) return rc;
    rc = forces(h, s);
    if (!rc && nbody::ext::on(h)) rc = nbody::ext::add<double>(h, s.sh, s.n_local, s.g, nullptr, false);
    return rc;
}

int set_integrator(NbodyHandle* h, int integrator) {   // (nbody_api.cpp has checked that the handle may run it)
    State& s = *h->f64;
    if (integrator == s.integrator) return NBODY_OK;
    if (integrator == NBODY_INTEGRATOR_HERMITE4) {
        int rc = ensure_hermite(h, s);
        if (rc) return rc;
    }
    s.integrator = integrator;
    s.hm_valid = false;
    s.lv_valid = false;
    if (integrator != NBODY_INTEGRATOR_HERMITE4) { s.blk_eta = 0.0; s.blk_L = 0; }   // block steps are a setting of a Hermite handle
    return NBODY_OK;
}

int set_block_steps(NbodyHandle* h, double eta, int max_level) {
    State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return fail(h, NBODY_ERR_INVALID, "nbody_set_block_steps: the handle runs the leapfrog integrator (nbody_set_integrator)");
    const bool off = eta == 0.0 && max_level == 0;
    if (!off && !(eta > 0.0 && max_level >= 1 && max_level <= 20))
        return fail(h, NBODY_ERR_INVALID, "nbody_set_block_steps: eta must be > 0 and max_level in 1..20, or (0, 0) to switch block steps off");
    if (!off) {
        int rc = ensure_block(h, s);
        if (rc) return rc;
    }
    s.blk_eta = off ? 0.0 : eta;
    s.blk_L = off ? 0 : max_level;
    s.lv_valid = false;
    return NBODY_OK;
}

int get_block_steps(const NbodyHandle* h, double* eta, int* max_level) {
    const State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return NBODY_ERR_INVALID;
    if (eta) *eta = s.blk_eta;
    if (max_level) *max_level = s.blk_L;
    return NBODY_OK;
}

int download_levels(NbodyHandle* h, int32_t* level, size_t cap, size_t* n_out) {
    State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return fail(h, NBODY_ERR_INVALID, "nbody_download_levels: the handle runs the leapfrog integrator (nbody_set_integrator)");
    if (s.blk_L == 0 || !s.hm_valid || !s.lv_valid)
        return fail(h, NBODY_ERR_INVALID, "nbody_download_levels: the levels are invalid (block steps are off, or the next step or nbody_update_forces assigns them)");
    int rc = s.sync_count(h, h->stream);
    if (rc) return rc;
    const size_t n = s.n_local;
    if (n_out) *n_out = n;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "download buffer too small");
    if (n == 0) return NBODY_OK;
    if (!level) return fail(h, NBODY_ERR_INVALID, "null buffer");
    static_assert(sizeof(int) == sizeof(int32_t), "levels are 32-bit");
    HIP_TRY(h, hipMemcpyAsync(level, s.blk.level, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}

int block_step_counts(NbodyHandle* h, uint64_t out[2]) {
    State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return fail(h, NBODY_ERR_INVALID, "nbody_block_step_counts: the handle runs the leapfrog integrator (nbody_set_integrator)");
    out[0] = s.blk_steps;
    out[1] = s.blk_updates;
    return NBODY_OK;
}

int debug_hermite_forces_of(NbodyHandle* h, const int32_t* ids, size_t n_ids, double* acc3, double* jerk3) {
    State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return fail(h, NBODY_ERR_INVALID, "nbody_debug_hermite_forces_of: the handle runs the leapfrog integrator (nbody_set_integrator)");
    int rc = s.sync_count(h, h->stream);
    if (rc) return rc;
    const size_t n = s.n_local;
    if (n_ids > n) return fail(h, NBODY_ERR_INVALID, "nbody_debug_hermite_forces_of: more ids than bodies (ids must be distinct and < n)");
    if (n_ids == 0) return NBODY_OK;
    if (!ids || !acc3 || !jerk3) return fail(h, NBODY_ERR_INVALID, "null buffer");
    std::vector<unsigned char> seen(n, 0);
    for (size_t k = 0; k < n_ids; ++k) {
        if (ids[k] < 0 || size_t(ids[k]) >= n || seen[size_t(ids[k])]) return fail(h, NBODY_ERR_INVALID, "nbody_debug_hermite_forces_of: ids must be distinct and < n");
        seen[size_t(ids[k])] = 1;
    }
    rc = ensure_block(h, s);
    if (rc) return rc;
    const int n_act = int(n_ids);
    const int head[2] = {0, n_act};   // (list, sched, planes, a1 and j1 are scratch that every block step rewrites)
    HIP_TRY(h, hipMemcpyAsync(s.blk.list, ids, n_ids * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(s.blk.sched, head, sizeof(head), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (pageable sources)
    HmActPlan plan;
    rc = hm_act_eval(h, s, s.sh.own_pos(), s.sh.vel, n_act, &plan);
    if (rc) return rc;
    if (h->cfg.math_mode == NBODY_MATH_FAST) launch_hm_act_reduce(h->stream, s.sh, s.hm, s.blk, plan, n_act, s.g);
    HIP_TRY(h, hipGetLastError());
    std::vector<double> ta(4 * n_ids), tj(4 * n_ids);
    HIP_TRY(h, hipMemcpyAsync(ta.data(), s.hm.a1, n_ids * sizeof(double4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(tj.data(), s.hm.j1, n_ids * sizeof(double4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < n_ids; ++k)
        for (int c = 0; c < 3; ++c) { acc3[3 * k + c] = ta[4 * k + c]; jerk3[3 * k + c] = tj[4 * k + c]; }
    return NBODY_OK;
}

int get_integrator(const NbodyHandle* h) { return h->f64->integrator; }

int download_jerk(NbodyHandle* h, double* jerk3, size_t cap, size_t* n_out) {
    State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return fail(h, NBODY_ERR_INVALID, "nbody_download_jerk: the handle runs the leapfrog integrator (nbody_set_integrator)");
    if (!s.hm_valid) return fail(h, NBODY_ERR_INVALID, "nbody_download_jerk: the held acceleration and jerk are stale (the next step or nbody_update_forces evaluates them)");
    int rc = s.sync_count(h, h->stream);
    if (rc) return rc;
    const size_t n = s.n_local;
    if (n_out) *n_out = n;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "download buffer too small");
    if (n == 0) return NBODY_OK;
    if (!jerk3) return fail(h, NBODY_ERR_INVALID, "null buffer");
    std::vector<double> tmp(4 * n);
    HIP_TRY(h, hipMemcpyAsync(tmp.data(), s.hm.jerk, n * sizeof(double4), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < n; ++k) { jerk3[3 * k] = tmp[4 * k]; jerk3[3 * k + 1] = tmp[4 * k + 1]; jerk3[3 * k + 2] = tmp[4 * k + 2]; }
    return NBODY_OK;
}

int suggest_dt(NbodyHandle* h, double eta, double* dt_out) {
    State& s = *h->f64;
    if (s.integrator != NBODY_INTEGRATOR_HERMITE4) return fail(h, NBODY_ERR_INVALID, "nbody_suggest_dt: the handle runs the leapfrog integrator (nbody_set_integrator)");
    if (!(eta > 0.0)) return fail(h, NBODY_ERR_INVALID, "nbody_suggest_dt: eta must be > 0");
    int rc = s.hm_valid ? NBODY_OK : hm_refresh(h, s);
    if (rc) return rc;
    double lowest = HUGE_VAL;
    const int blocks = launch_hm_min_ratio(h->stream, s.sh, s.hm, int(s.n_local));
    if (blocks > 0) {
        HIP_TRY(h, hipGetLastError());
        std::vector<double> part(static_cast<size_t>(blocks));
        HIP_TRY(h, hipMemcpyAsync(part.data(), s.hm.ratio, size_t(blocks) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (double r : part) lowest = std::min(lowest, r);
    }
    *dt_out = eta * lowest;
    return NBODY_OK;
}

int stats(NbodyHandle* h, NbodyStats* out) { return engine::stats(h, *h->f64, out); }

int reset_stats(NbodyHandle* h) {
    h->f64->blk_steps = 0; h->f64->blk_updates = 0;
    return engine::reset_stats(h, *h->f64);
}

int energy(NbodyHandle* h, double* kinetic, double* potential) {
    State& s = *h->f64;
    if (s.sh.n_seg > 1) return fail(h, NBODY_ERR_INVALID, "nbody_energy on a sharded f64 world is not supported (a rank holds the velocities of its own block only)");
    return engine::energy(h, s, kinetic, potential);
}

// nbody_potentials / nbody_energy_world on an f64 handle (nbody_f32.cpp potentials_device is the f32 twin and has the contract)
int potentials_device(NbodyHandle* h, int mode, size_t* n_own, nbody::PotBodies* bodies, double* g, bool field) {
    State& s = *h->f64;
    if (mode == NBODY_POTENTIAL_TREE && !s.bounds_set) return fail(h, NBODY_ERR_INVALID, "nbody_set_bounds has not been called");
    int rc = exchange(h, s);   // sharded: every block's current positions and live count
    if (rc) return rc;
    engine::PotView<double> view(s);   // (the host's view of the counts: exact for the call, put back when it ends)
    rc = view.begin(h, bodies, g);
    if (!rc && mode == NBODY_POTENTIAL_PAIRS) {
        if (!field) rc = nbody::pot::pairs(h, *bodies, s.n_local, engine::total_upper(s) - s.n_local, s.g_soft * s.g_soft);
    } else if (!rc) {
        PotWalkScope walking(h->pot, field ? kWalkField : kWalkPotentials);
        rc = bh_forces(h, s);
    }
    *n_own = s.n_local;
    return rc ? rc : comm_check(h);
}

}  // namespace nbody64
