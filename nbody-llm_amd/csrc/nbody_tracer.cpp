// nbody_tracer.cpp -- tracers: massless particles that ride in the bodies' field (include/nbody_hip.h, "tracers").
//
// The tracer vector is a second nbody::Shard of one segment (TracerState::sh): half drift, retain and kick + half drift are
// the bodies' kernels on that struct; the force pass is one-sided, tracers x bodies (kernels_tracer.hip).  Everything is
// enqueued on the handle's stream; the live tracer count stays on the device and launches are sized from the host's upper
// bound, as for the bodies.
#include "nbody_tracer.h"
#include "nbody_f32.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace nbody { namespace tracer {

const char* refusal(const NbodyHandle* h) {
    if (h->cfg.dtype != NBODY_F32) return "tracers need an NBODY_F32 handle (NBODY_F64 is out of scope)";
    if (h->cfg.world_size != 1) return "tracers need a world_size == 1 handle (multi-rank worlds are out of scope)";
    return nullptr;
}

namespace {

// the statistics words: {accepted or directed interactions, opening tests} pairs the walk's waves are spread over (the
// brute-force passes add to the first pair only); summed by the reader
constexpr size_t kStatWords = 2 * size_t(NBODY_WALK_COUNTER_SLOTS);

// arrays for `cap` tracers (replaces smaller ones; the contents are the caller's to fill) and the statistics words
int ensure(NbodyHandle* h, size_t cap) {
    auto& b = nbody32::bodies(h);
    TracerState& t = h->tr;
    if (!t.d_stats) {
        HIP_TRY(h, h->mem.dev(t.d_stats, kStatWords * sizeof(unsigned long long)));
        HIP_TRY(h, hipMemsetAsync(t.d_stats, 0, kStatWords * sizeof(unsigned long long), h->stream));
    }
    if (cap <= t.cap) return NBODY_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    shard_free(h, t.sh);
    t.cap = 0;
    Shard& sh = t.sh;
    sh.n_seg = 1; sh.my_seg = 0; sh.seg_cap = int(cap);
    sh.poison = b.sh.poison;   // (steps enqueued without read-back: the half drift and the retain stop with the bodies')
    const int rc = shard_alloc(h, h->stream, sh, false);   // (no interaction counter: the statistics words above)
    if (rc) return rc;
    t.cap = cap;
    return NBODY_OK;
}

// the host's view of the live tracer count made exact (one 4-byte read-back), only when it may be stale
int sync_count(NbodyHandle* h) {
    TracerState& t = h->tr;
    if (!t.dirty || !t.sh.seg_count) return NBODY_OK;
    int* hv = h->h_poison + kScratchTracerCount;
    HIP_TRY(h, hipMemcpyAsync(hv, t.sh.seg_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    t.n_host = size_t(*hv);
    t.dirty = false;
    return NBODY_OK;
}

}  // namespace

int upload(NbodyHandle* h, const void* aos, size_t n, size_t stride, size_t capacity) {
    auto& b = nbody32::bodies(h);
    TracerState& t = h->tr;
    const size_t cap = capacity ? capacity : n;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_tracers_upload: more tracers than the capacity given");
    if (cap > (size_t(1) << 30)) return fail(h, NBODY_ERR_CAPACITY, "nbody_tracers_upload: capacity must be at most 2^30");
    if (cap == 0) {   // the empty set and no room asked for: the handle is as if it never had tracers
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        unsigned long long* keep_stats = t.d_stats;
        shard_free(h, t.sh);
        h->mem.free_dev(t.d_planes); h->mem.free_dev(t.d_keys); h->mem.free_dev(t.d_idx); h->mem.free_dev(t.d_sort_tmp); h->mem.free_dev(t.d_info);
        t = TracerState{};
        t.d_stats = keep_stats;
        return NBODY_OK;
    }
    int rc = ensure(h, cap);
    if (!rc) rc = b.ensure_aos(h, n);
    if (rc) return rc;
    const char* src = static_cast<const char*>(aos);
    for (size_t k = 0; k < n; ++k) {
        std::memcpy(b.h_aos + 10 * k, src + k * stride, 36);
        b.h_aos[10 * k + 9] = 0.f;   // the mass field is ignored: a tracer has none
    }
    if (n) HIP_TRY(h, hipMemcpyAsync(b.d_aos, b.h_aos, n * 40, hipMemcpyHostToDevice, h->stream));
    nbody::launch_aos_to_soa(h->stream, b.d_aos, 10, int(n), t.sh.pos_all, t.sh.vel, t.sh.acc);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemsetAsync(t.sh.escaped, 0, sizeof(int), h->stream));
    int* hv = h->h_poison + kScratchTracerCount;
    *hv = int(n);
    HIP_TRY(h, hipMemcpyAsync(t.sh.seg_count, hv, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the staging buffers are reused
    t.n_host = n;
    t.n_plan = n;
    t.dirty = false;
    return NBODY_OK;
}

int download(NbodyHandle* h, void* aos, size_t cap, size_t stride, size_t* n_out) {
    auto& b = nbody32::bodies(h);
    int rc = sync_count(h);
    if (rc) return rc;
    TracerState& t = h->tr;
    const size_t n = t.n_host;
    if (n_out) *n_out = n;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_tracers_download: buffer too small");
    if (n == 0) return NBODY_OK;
    if (!aos) return fail(h, NBODY_ERR_INVALID, "nbody_tracers_download: null buffer");
    rc = b.ensure_aos(h, n);
    if (rc) return rc;
    nbody::launch_soa_to_aos(h->stream, b.d_aos, 10, int(n), t.sh.pos_all, t.sh.vel, t.sh.acc);   // (pos.w = 0: the mass written)
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(b.h_aos, b.d_aos, n * 40, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    char* dst = static_cast<char*>(aos);
    for (size_t k = 0; k < n; ++k) std::memcpy(dst + k * stride, b.h_aos + 10 * k, 40);
    return NBODY_OK;
}

int count(NbodyHandle* h, size_t* n_out) {
    int rc = sync_count(h);
    if (rc) return rc;
    *n_out = h->tr.n_host;
    return NBODY_OK;
}

int stats(NbodyHandle* h, uint64_t out[2]) {
    out[0] = out[1] = 0;
    if (!h->tr.d_stats) return NBODY_OK;
    std::vector<unsigned long long> words(kStatWords);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(words.data(), h->tr.d_stats, kStatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < kStatWords; k += 2) { out[0] += words[k]; out[1] += words[k + 1]; }
    return NBODY_OK;
}

int reset_stats(NbodyHandle* h) {
    if (h->tr.d_stats) HIP_TRY(h, hipMemsetAsync(h->tr.d_stats, 0, kStatWords * sizeof(unsigned long long), h->stream));
    return NBODY_OK;
}

int clone_state(const NbodyHandle* src, NbodyHandle* dst) {
    const TracerState& a = src->tr;
    if (!a.cap) return NBODY_OK;
    int rc = ensure(dst, a.cap);
    if (rc) return rc;
    TracerState& b = dst->tr;
    HIP_TRY(dst, hipMemcpyAsync(b.sh.pos_all, a.sh.pos_all, a.cap * sizeof(float4), hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(dst, hipMemcpyAsync(b.sh.vel, a.sh.vel, a.cap * sizeof(float4), hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(dst, hipMemcpyAsync(b.sh.acc, a.sh.acc, a.cap * sizeof(float4), hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(dst, hipMemcpyAsync(b.sh.seg_count, a.sh.seg_count, sizeof(int), hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    b.n_host = a.n_host;   // (the same upper bound: the clone's launches are its source's)
    b.n_plan = a.n_plan;   // (and the same plans)
    b.dirty = a.dirty;
    return NBODY_OK;
}

int drift_retain(NbodyHandle* h, float dt) {
    auto& b = nbody32::bodies(h);
    if (!on(h)) return NBODY_OK;
    TracerState& t = h->tr;
    nbody::launch_drift_half(h->stream, t.sh, int(t.n_host), dt, b.bnd);
    nbody::launch_compact(h->stream, t.sh, int(t.n_host));
    t.dirty = true;
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

int forces(NbodyHandle* h, const float* kick_dt) {
    auto& b = nbody32::bodies(h);
    if (!on(h)) return NBODY_OK;
    TracerState& t = h->tr;
    const float eps2 = b.g_soft * b.g_soft;
    const int m = int(t.n_host);
    if (h->cfg.math_mode == NBODY_MATH_STRICT) {
        nbody::launch_tr_bf_strict(h->stream, t.sh, m, b.sh, b.g, eps2, t.d_stats);
        if (kick_dt) nbody::launch_kick_drift(h->stream, t.sh, m, *kick_dt);
    } else {
        // the plan is drawn from the counts at the uploads of the tracers and of the bodies, not from the host's current view
        // of them, which a read-back after an escape refreshes: the slice partition, and with it the bits, do not depend on
        // when the caller looks
        const nbody::TracerPlan p = nbody::tracer_plan(t.n_plan, std::max(h->n_at_upload, b.n_local));
        if (p.K > 1) {
            const size_t need = size_t(p.K) * nbody::tracer_plan_pad(p);
            HIP_TRY(h, grow_dev(h, t.d_planes, t.planes_cap, need, sizeof(float4), Grow::exact, kGrowSync));
        }
        nbody::launch_tr_bf_fast(h->stream, t.sh, m, b.sh, p, t.d_planes, b.g, eps2, kick_dt, t.d_stats);
    }
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

// Barnes-Hut: called by the body force pass right after its walk, with the tree it built (nothing has overwritten it yet).
// The tracers are keyed and sorted into tree order, then walk td's nodes over td's split points; the kick + half drift of a
// step ride in the walk or in its reduction.  Everything is enqueued: the device build's steps stay without a read-back.
int tree_forces(NbodyHandle* h, const nbody::TreeDev& td, const float* kick_dt) {
    auto& b = nbody32::bodies(h);
    if (!on(h)) return NBODY_OK;
    TracerState& t = h->tr;
    const int m = int(t.n_host);
    if (t.sort_cap < t.cap) {   // the sort's buffers, sized for the capacity once
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        t.sort_cap = 0;   // (three blocks under one cap: each replaces its old one)
        t.sort_bytes = std::max<size_t>(nbody::tracer_sort_tmp_bytes(t.cap), 256);
        HIP_TRY(h, h->mem.dev(t.d_keys, 2 * t.cap * sizeof(unsigned long long)));
        HIP_TRY(h, h->mem.dev(t.d_idx, 2 * t.cap * sizeof(int)));
        HIP_TRY(h, h->mem.dev(t.d_sort_tmp, t.sort_bytes));
        if (!t.d_info) HIP_TRY(h, h->mem.dev(t.d_info, 3 * sizeof(int)));
        t.sort_cap = t.cap;
    }
    const int* idx = nullptr;
    if (nbody::tracer_sort(h->stream, t.sh.own_pos(), t.sh.own_count(), m, b.center, b.width, t.d_sort_tmp, t.sort_bytes, t.d_keys, t.d_idx,
                           t.sort_cap, t.d_info, &idx) != 0)
        return fail(h, NBODY_ERR_HIP, "tracer force pass: rocPRIM call failed");
    // (runs drawn from the upload-time count, like the brute-force plan: see forces)
    const int groups = nbody::tracer_walk_groups(t.n_plan, td.n_split);
    const size_t stride = (t.cap + 63) / 64 * 64;
    if (groups > 1) {
        HIP_TRY(h, grow_dev(h, t.d_planes, t.planes_cap, size_t(groups) * stride, sizeof(float4), Grow::exact, kGrowSync));
    }
    nbody::launch_tr_bh_walk(h->stream, t.sh, m, idx, td, groups, t.d_planes, stride, b.g, b.g_soft * b.g_soft, b.theta2,
                             h->cfg.leaf_mode == NBODY_LEAF_DIRECT, kick_dt, t.d_stats);
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

}}  // namespace nbody::tracer
