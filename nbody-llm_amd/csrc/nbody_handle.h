// nbody_handle.h -- the handle behind include/nbody_hip.h (internal to libnbody_hip.so).  The handle itself holds nothing of a
// precision: the bodies, their settings and the tree are its engine's (EngineBodies<F> below; nbody_f32.h / nbody_f64.h bodies(h)).
#pragma once
#include "../../include/nbody_hip.h"
#include "kernels.h"
#include "kernels_f64.h"
#include "kernels_quad.h"
#include "octree_host.h"
#include "handle_mem.h"

#include "transport.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

using nbody::BoundsF;
using nbody::Shard;

namespace nbody32 { struct State; }   // F = f32 handles (nbody_f32.cpp)
namespace nbody64 { struct State; }   // F = f64 handles (nbody_f64.cpp)
namespace nbody { namespace let { struct State; } }   // spatial shards (nbody_let.cpp)
struct NbodyHandle;

// ---- host helpers of every translation unit behind the handle

// records msg as the handle's error (h == nullptr: as nbody_create's) and returns code (nbody_api.cpp)
int fail(NbodyHandle* h, int code, const std::string& msg);
// anything the transport noticed behind the host's back (a device-side wait that ran out of time, a peer that gave up), as the
// handle's error (nbody_api.cpp)
int comm_check(NbodyHandle* h);

// (expr: a hipError_t, or the int a HandleMem operation hands through from the seam below)
#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = hipError_t(expr);                                                                     \
        if (e_ != hipSuccess)                                                                         \
            return fail(h, NBODY_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

#define TP_TRY(h, expr)                                                                               \
    do {                                                                                              \
        int r_ = (expr);                                                                              \
        if (r_ != NBODY_OK) return fail(h, r_, std::string(#expr) + ": " + (h)->tp->error());         \
    } while (0)

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// ---- memory: every device and pinned block of a handle is taken from and given back to its HandleMem (NbodyHandle::mem), which
// reaches the runtime through this seam and nowhere else; free_all releases whatever is live in one call
inline int hip_dev_alloc(void** p, size_t n) { return int(hipMalloc(p, n)); }
inline void hip_dev_free(void* p) { (void)hipFree(p); }
inline int hip_pin_alloc(void** p, size_t n) { return int(hipHostMalloc(p, n, hipHostMallocDefault)); }
inline void hip_pin_free(void* p) { (void)hipHostFree(p); }
constexpr nbody::MemSeam kHipSeam{hip_dev_alloc, hip_dev_free, hip_pin_alloc, hip_pin_free};
using nbody::Grow;
nbody::HandleMem& mem_of(NbodyHandle* h);   // h->mem, for the structures declared before the handle

// the host octree's node arrays (HostTreeT's allocator hooks carry no context): pinned through the same seam, owned and freed
// by the HostTreeT itself
inline void* pinned_alloc(size_t n) {
    void* p = nullptr;
    return hip_pin_alloc(&p, n) == 0 ? p : nullptr;
}
inline void pinned_free(void* p) { hip_pin_free(p); }

// ---- the Barnes-Hut walk's node-range split (kernels.h kMaxSplit: the layout of its int array), for f32 and f64 walks:
// the buffers, the number of segments, the listing of the split points' ancestors, the walk's view of them

// segments of a walk over n_walk bodies: walk_plan's, halved while a segment would hold fewer than 16 of n_bound nodes;
// strict math walks in one piece (the reference's sum order); a pinned NBODY_BH_SPLIT is taken as given; no bodies: one
inline nbody::WalkPlan walk_split_plan(size_t n_walk, bool fast_math, float theta2, size_t n_bound) {
    nbody::WalkPlan p = nbody::walk_plan(n_walk, fast_math, nbody::kMaxSplit, theta2);
    const bool pinned = nbody::tuning().bh_walk_split > 0;
    if (!fast_math && !pinned) p.segments = 1;
    while (!pinned && p.segments > 1 && size_t(p.segments) * 16 > n_bound) p.segments /= 2;
    if (n_walk == 0) p.segments = 1;
    return p;
}

// nbody_field_at(TREE): segments of the walk over a call's probes.  The field walk runs one probe per lane and never more than
// kFieldBatch probes per launch, so K is sized for the first batch at one per lane (walk_plan's one-body rule: ~16 384 waves),
// not from the probe total or the force walk's bodies-per-lane heuristic; pinned NBODY_BH_SPLIT as given; chosen once per call
constexpr size_t kFieldBatch = 65536;
inline int field_split_plan(size_t n_points, size_t n_bound) {
    if (n_points == 0) return 1;
    if (nbody::tuning().bh_walk_split > 0) return std::min(nbody::tuning().bh_walk_split, nbody::kMaxSplit);
    const size_t waves = (std::min(n_points, kFieldBatch) + 63) / 64;
    int K = int(std::min<size_t>(size_t(nbody::kMaxSplit), (16384 + waves - 1) / waves));
    while (K > 1 && size_t(K) * 16 > n_bound) K /= 2;
    return std::max(K, 1);
}

template <class V>   // float4 (f32 walk) or double4 (f64): the segments' partial sums
struct WalkSplitBuf {
    int* d = nullptr;        // [kSplitInts] first[] | n_anc[] | anc[][]
    int* h = nullptr;        // pinned mirror (ancestors listed on the host)
    V* planes = nullptr;     // [K][stride] partial sums of the segments, grow-only
    size_t planes_cap = 0;   // V entries

    int* first() const { return d; }
    int* n_anc() const { return d + nbody::kMaxSplit + 1; }
    int* anc() const { return d + 2 * nbody::kMaxSplit + 1; }

    // the int array, and planes for K segments of `stride` bodies
    int ensure(NbodyHandle* hh, int K, size_t stride) {
        if (!d) {
            HIP_TRY(hh, mem_of(hh).dev(d, nbody::kSplitInts * sizeof(int)));
            HIP_TRY(hh, mem_of(hh).pin(h, nbody::kSplitInts * sizeof(int)));
        }
        if (K > 1) HIP_TRY(hh, mem_of(hh).grow(planes, planes_cap, size_t(K) * stride, sizeof(V), Grow::exact));
        return NBODY_OK;
    }
    // K equal parts of a host-built tree's n_nodes; the ancestors of each split point found down from the root along the skip links
    template <class F>
    int list_on_host(NbodyHandle* hh, hipStream_t s, const nbody::NodeRecT<F>* nodes, int n_nodes, int K) {
        int* hf = h;
        int* hn = h + nbody::kMaxSplit + 1;
        int* ha = h + 2 * nbody::kMaxSplit + 1;
        for (int k = 0; k <= K; ++k) hf[k] = int((long long)n_nodes * k / K);
        for (int k = 0; k < K; ++k) {
            int cnt = 0, j = 0;
            const int target = hf[k];
            while (j != target && cnt < nbody::kMaxAnc) {
                ha[k * nbody::kMaxAnc + cnt++] = j;   // j < target < skip(j): an ancestor
                int c = j + 1;                        // its first child
                while (nodes[c].b.skip <= target) c = nodes[c].b.skip;   // siblings in orthant order
                j = c;
            }
            hn[k] = cnt;
        }
        HIP_TRY(hh, hipMemcpyAsync(d, h, (2 * size_t(nbody::kMaxSplit) + 1 + size_t(K) * nbody::kMaxAnc) * sizeof(int), hipMemcpyHostToDevice, s));
        return NBODY_OK;
    }
    // the same from the device build's arrays (info != nullptr: its node and body counts are read on the device)
    void list_on_device(hipStream_t s, const nbody::TreeDevWork& work, int n, int n_nodes, int K, const int* info = nullptr, int* poison = nullptr) const {
        nbody::launch_tree_split_anc(s, work, n, n_nodes, K, first(), n_anc(), anc(), nbody::kMaxAnc, info, poison);
    }
    // ... or in the build's last launch
    nbody::TreeSplitReq request(int K, const int* info, int* poison) const {
        nbody::TreeSplitReq r;
        r.n_split = K; r.first = first(); r.n_anc = n_anc(); r.anc = anc(); r.max_anc = nbody::kMaxAnc; r.info = info; r.poison = poison;
        return r;
    }
};

// the walks' views of K segments
inline void walk_split_view(const WalkSplitBuf<float4>& b, int K, size_t stride, nbody::TreeDev* td) {
    td->n_split = K;
    td->split_first = b.first(); td->split_n_anc = b.n_anc(); td->split_anc = b.anc();
    if (K > 1) { td->split_planes = b.planes; td->split_stride = stride; }
}
inline nbody64::WalkSplit64 walk_split_view(const WalkSplitBuf<double4>& b, int K, size_t stride) {
    return nbody64::WalkSplit64{K, b.first(), b.anc(), b.n_anc(), b.planes, stride};
}

// ---- the device build's buffers (kernels_tree.hip), f32 and f64
struct TreeBuildBufs {
    void* ws = nullptr;        // workspace (keys, sort buffers, scans)
    void* cat = nullptr;       // sharded worlds: concatenated positions, own-order list
    size_t cap = 0;            // bodies both are sized for
    int* d_info = nullptr;     // [4] node count, flags, bodies in the tree
    int* h_info = nullptr;     // pinned

    // for n_cap bodies; cat_bytes = 0: no concatenation buffer (one shard)
    int ensure(NbodyHandle* hh, size_t n_cap, size_t cat_bytes) {
        if (cap < n_cap) {   // (two blocks under one cap: each replaces its old one)
            cap = 0;
            HIP_TRY(hh, mem_of(hh).dev(ws, nbody::tree_build_workspace_bytes(n_cap)));
            mem_of(hh).free_dev(cat);
            if (cat_bytes) HIP_TRY(hh, mem_of(hh).dev(cat, cat_bytes));
            cap = n_cap;
        }
        if (!d_info) {
            HIP_TRY(hh, mem_of(hh).dev(d_info, 4 * sizeof(int)));
            HIP_TRY(hh, mem_of(hh).pin(h_info, 4 * sizeof(int)));
        }
        return NBODY_OK;
    }
};

// nbody_potentials / nbody_energy_world (nbody_pot.cpp): buffers of their own -- a call writes none of the force pass's
enum { kWalkForces = 0, kWalkPotentials = 1, kWalkField = 2 };   // PotBufs::walking
struct PotBufs {
    int walking = kWalkForces;    // kWalkPotentials: an NBODY_POTENTIAL_TREE call is under way: the force pass builds its tree as usual
                                  // and its last phase walks for potentials (always over the node-range split, DIRECT leaf rule);
                                  // kWalkField: nbody_field_at(TREE): the last phase leaves the tree's view in FieldBufs instead
    bool quad = false;            // the call under way is in NBODY_POTENTIAL_TREE_QUADRUPOLE: the last phase fills NbodyHandle::d_quad from
                                  // the tree it has just built and walks with the quadrupole kernels (kernels_quad.hip)
    double* d_sum = nullptr;      // [sum_cap] S_i = sum m_j / sqrt(r2 + eps2) per own body, indexed like the own segment
    size_t sum_cap = 0;
    double* d_planes = nullptr;   // partial sums of the walk's segments / the pair kernels' slices, grow-only
    size_t planes_cap = 0;        // doubles
    unsigned long long* d_counts = nullptr;   // [NBODY_WALK_COUNTER_SLOTS][2] accepted, visited of the call under way
    unsigned long long* h_counts = nullptr;   // pinned
    double* d_part = nullptr;     // [2 * part_blocks] per-block {KE, sum m S}
    size_t part_blocks = 0;
    // spatial shards: the sums travel from the ranks that walked the bodies back to their owners (kernels_pot.h PotRec)
    void* d_rec = nullptr;        // [world][seg_cap] records, all-gathered
    size_t rec_cap = 0;           // records
    int* d_rec_count = nullptr;   // [world]
    int* d_slot_of = nullptr;     // [slot_cap] index in the uploaded vector -> own slot, -1
    size_t slot_cap = 0;
};

// the only way PotBufs::walking is set: for the lifetime of this object, so that no return path of a force pass run for
// potentials can leave the handle walking for potentials when the next step comes
struct PotWalkScope {
    PotBufs& p;
    explicit PotWalkScope(PotBufs& pb, int what = kWalkPotentials, bool quad = false) : p(pb) { p.walking = what; p.quad = quad; }
    ~PotWalkScope() { p.walking = kWalkForces; p.quad = false; }
    PotWalkScope(const PotWalkScope&) = delete;
    PotWalkScope& operator=(const PotWalkScope&) = delete;
};

// nbody_field_at (nbody_field.cpp): probes go through the device in batches of at most kFieldBatch, so the scratch is bounded:
// planes of [K <= 64][batch]{ax, ay, az, S} doubles are at most 64 * 65 536 * 32 B = 128 MiB (nbody_tidal_at: six doubles a
// row, 192 MiB).  Grown on demand, not cloned.
struct FieldBufs {
    size_t n_points = 0;          // probes of the call under way: the walk's split count K is drawn from it, once per call
    // the tree the call's force pass built, as its last phase left it (valid until the next force pass)
    const void* nodes = nullptr;  // NodeDev (f32) or Node64 (f64) records
    int n_nodes = 0, K = 1;
    const float4* quad = nullptr; // NBODY_POTENTIAL_TREE_QUADRUPOLE: that tree's tensors (NbodyHandle::d_quad), else null
    const int* first = nullptr;   // the split's arrays (WalkSplitBuf)
    const int* anc = nullptr;
    const int* n_anc = nullptr;
    // per-batch scratch, all for kFieldBatch probes
    double* d_xyz = nullptr;                  // [batch][3] the caller's points
    unsigned long long* d_keys = nullptr;     // [2][batch] Morton keys, unsorted | sorted
    int* d_idx = nullptr;                     // [2][batch] place in the batch, unsorted | sorted
    void* d_sort_tmp = nullptr;
    size_t sort_bytes = 0;
    double* d_out = nullptr;                  // [batch][3] accelerations | [batch] potentials; nbody_tidal_at: [batch][6]
    size_t out_cap = 0;                       // doubles: 4 per probe until the first nbody_tidal_at, 6 from then on
    double* d_planes = nullptr;               // [K][stride] double4 partial sums, grow-only
    size_t planes_cap = 0;                    // doubles
};

// how a handle's bodies are sharded (NbodyHandle::shape, drawn by nbody_api.cpp create_impl): index blocks, or the one
// segment of a spatial rank
struct ShardShape { int n_seg = 1, my_seg = 0, seg_cap = 0; };

// ---- the body vector of a handle, for F = f32 and F = f64 (a base of EngineBodies<F> below): the
// device arrays, the host's view of them, the settings, and the Vec-like operations that do not depend on how the forces are
// computed.  The members take the handle (for errors) and the stream they enqueue on.

// contiguous index blocks of a vector of n bodies over G shards (they keep the ascending-partner order): block g is [lo, hi)
inline void index_block(size_t n, size_t G, size_t g, size_t* lo, size_t* hi) {
    const size_t blk = (n + G - 1) / G;
    *lo = std::min(n, g * blk);
    *hi = std::min(n, *lo + blk);
}

// The arrays of a shard (the bodies' and the tracers') for its n_seg / seg_cap, zeroed (keep flags 1, epoch 1: the zeroed status
// words belong to no launch); `inter` only when asked for; poison and ids stay as they are.  Enqueues the fills on s: the caller
// synchronises.  shard_free gives the same arrays back and leaves an empty shard.
template <class F>
int shard_alloc(NbodyHandle* h, hipStream_t s, nbody::ShardT<F>& sh, bool with_inter) {
    using V4 = typename nbody::ShardT<F>::V4;
    const size_t cap = size_t(sh.seg_cap), G = size_t(sh.n_seg);
    const size_t tiles = (cap + 1023) / 1024 + 1;
    nbody::HandleMem& mem = mem_of(h);
    const auto arr = [&](auto*& p, size_t bytes, int fill) {
        HIP_TRY(h, mem.dev(p, bytes));
        HIP_TRY(h, hipMemsetAsync(p, fill, bytes, s));
        return int(NBODY_OK);
    };
    int rc = arr(sh.pos_all, G * cap * sizeof(V4), 0);
    if (!rc) rc = arr(sh.vel, cap * sizeof(V4), 0);
    if (!rc) rc = arr(sh.acc, cap * sizeof(V4), 0);
    if (!rc) rc = arr(sh.seg_count, G * sizeof(int), 0);
    if (!rc) rc = arr(sh.escaped, sizeof(int), 0);
    if (!rc) rc = arr(sh.keep, cap, 1);
    if (!rc) rc = arr(sh.tile_state, tiles * sizeof(unsigned long long), 0);
    if (!rc) rc = arr(sh.epoch, sizeof(int), 0);
    if (!rc && with_inter) rc = arr(sh.inter, sizeof(unsigned long long), 0);
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(sh.epoch, 1, 1, s));   // epoch = 1
    return NBODY_OK;
}
template <class F>
void shard_free(NbodyHandle* h, nbody::ShardT<F>& sh) {
    nbody::HandleMem& mem = mem_of(h);
    mem.free_dev(sh.pos_all); mem.free_dev(sh.vel); mem.free_dev(sh.acc); mem.free_dev(sh.seg_count); mem.free_dev(sh.escaped);
    mem.free_dev(sh.keep); mem.free_dev(sh.tile_state); mem.free_dev(sh.epoch); mem.free_dev(sh.inter);
    sh = nbody::ShardT<F>{};
}

template <class F>
struct BodyStore {
    using V4 = typename nbody::ShardT<F>::V4;
    static constexpr size_t kRecBytes = 10 * sizeof(F);   // one PointParticle<F,3> record: pos, vel, acc, mass

    nbody::ShardT<F> sh;
    F g = F(1), g_soft = F(0), dt = F(1e-3), theta2 = F(0.5);  // shared.rs:69-78
    F center[3] = {F(0), F(0), F(0)};
    F width = F(0);
    typename nbody::RealTypes<F>::Bounds bnd{};
    bool bounds_set = false;
    F elapsed = F(0);

    size_t n_local = 0;        // host view of the own body count (an upper bound while count_dirty)
    bool count_dirty = false;  // drift may have dropped bodies since n_local was read
    std::vector<int> seg_count_host;  // host view of every segment's count (upper bounds likewise; counts only shrink between uploads)
    int* h_counts = nullptr;   // pinned [n_seg]: all segments' counts on their way up or down

    F* d_aos = nullptr;        // device staging for PointParticle records (bodies and tracers alike), grow-only
    F* h_aos = nullptr;        // pinned host staging
    size_t aos_cap = 0;        // records

    // the arrays of sh in the handle's shape (shard_alloc: the caller synchronises) and the pinned counts
    int alloc(NbodyHandle* h, hipStream_t s, const ShardShape& shape) {
        sh.n_seg = shape.n_seg; sh.my_seg = shape.my_seg; sh.seg_cap = shape.seg_cap;
        const int rc = shard_alloc(h, s, sh, true);
        if (rc) return rc;
        HIP_TRY(h, mem_of(h).pin(h_counts, size_t(sh.n_seg) * sizeof(int)));
        seg_count_host.assign(size_t(sh.n_seg), 0);
        return NBODY_OK;
    }
    // what a clone takes over from `a` (same shape): the bodies of every segment and their counts, enqueued on s once the
    // caller has synchronised a's stream, and the host view.  Like the reference's BH clone (barnes_hut.rs:113-135), no tree.
    int copy_from(NbodyHandle* h, hipStream_t s, const BodyStore& a) {
        const size_t cap = size_t(a.sh.seg_cap), G = size_t(a.sh.n_seg);
        HIP_TRY(h, hipMemcpyAsync(sh.pos_all, a.sh.pos_all, G * cap * sizeof(V4), hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(sh.vel, a.sh.vel, cap * sizeof(V4), hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(sh.acc, a.sh.acc, cap * sizeof(V4), hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(sh.seg_count, a.sh.seg_count, G * sizeof(int), hipMemcpyDeviceToDevice, s));
        g = a.g; g_soft = a.g_soft; dt = a.dt; theta2 = a.theta2;
        std::copy(a.center, a.center + 3, center);
        width = a.width; bnd = a.bnd; bounds_set = a.bounds_set;
        elapsed = a.elapsed;
        n_local = a.n_local;
        seg_count_host = a.seg_count_host;
        return NBODY_OK;
    }

    // staging for `records` PointParticle records: device and pinned host, grow-only
    int ensure_aos(NbodyHandle* h, size_t records) {
        if (records <= aos_cap) return NBODY_OK;
        aos_cap = 0;   // (the device block and its pinned mirror under one cap: each replaces its old one)
        HIP_TRY(h, mem_of(h).dev(d_aos, records * kRecBytes));
        HIP_TRY(h, mem_of(h).pin(h_aos, records * kRecBytes));
        aos_cap = records;
        return NBODY_OK;
    }
    // refresh the host view of the counts (one small D2H + sync), only when it may be stale
    int sync_count(NbodyHandle* h, hipStream_t s) {
        if (!count_dirty) return NBODY_OK;
        HIP_TRY(h, hipMemcpyAsync(h_counts, sh.seg_count, sizeof(int) * sh.n_seg, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        for (int k = 0; k < sh.n_seg; ++k) seg_count_host[size_t(k)] = h_counts[k];
        n_local = size_t(h_counts[sh.my_seg]);
        count_dirty = false;
        return NBODY_OK;
    }
    // the host's counts of every segment / n_local as the own segment's count to the device; synchronises (h_counts is reused)
    int push_counts(NbodyHandle* h, hipStream_t s) {
        for (int k = 0; k < sh.n_seg; ++k) h_counts[k] = seg_count_host[size_t(k)];
        HIP_TRY(h, hipMemcpyAsync(sh.seg_count, h_counts, sizeof(int) * sh.n_seg, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        return NBODY_OK;
    }
    int push_own_count(NbodyHandle* h, hipStream_t s) {
        h_counts[sh.my_seg] = int(n_local);
        HIP_TRY(h, hipMemcpyAsync(sh.own_count(), h_counts + sh.my_seg, sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        return NBODY_OK;
    }

    void set_settings(F g_, F g_soft_, F dt_, F theta2_) { g = g_; g_soft = g_soft_; dt = dt_; theta2 = theta2_; }
    template <class T> void get_settings(T* g_, T* g_soft_, T* dt_, T* theta2_) const {
        if (g_) *g_ = T(g);
        if (g_soft_) *g_soft_ = T(g_soft);
        if (dt_) *dt_ = T(dt);
        if (theta2_) *theta2_ = T(theta2);
    }
    void set_bounds(const F c[3], F w) {
        std::copy(c, c + 3, center);
        width = w;
        const F hw = width * F(0.5);  // Bounds::new
        for (int i = 0; i < 3; ++i) {
            bnd.lo[i] = center[i] + (-hw);  // add_scalar(-half_width), shared.rs:224
            bnd.hi[i] = center[i] + hw;     // shared.rs:228
        }
        bounds_set = true;
    }

    // the caller's n records of `stride` bytes into the index blocks: every block's positions, the own block's velocities and
    // accelerations; *own_first = where the own block starts in the vector (its length is n_local).  Synchronises.
    int upload_blocks(NbodyHandle* h, hipStream_t s, const void* aos, size_t n, size_t stride, size_t* own_first) {
        int rc = ensure_aos(h, n);
        if (rc) return rc;
        const char* src = static_cast<const char*>(aos);
        for (size_t k = 0; k < n; ++k) std::memcpy(h_aos + 10 * k, src + k * stride, kRecBytes);
        if (n) HIP_TRY(h, hipMemcpyAsync(d_aos, h_aos, n * kRecBytes, hipMemcpyHostToDevice, s));
        for (size_t k = 0; k < size_t(sh.n_seg); ++k) {
            size_t lo, hi;
            index_block(n, size_t(sh.n_seg), k, &lo, &hi);
            seg_count_host[k] = int(hi - lo);
            const bool own = int(k) == sh.my_seg;
            nbody::launch_aos_to_soa<F>(s, d_aos + 10 * lo, 10, int(hi - lo), sh.pos_all + k * size_t(sh.seg_cap), own ? sh.vel : nullptr,
                                        own ? sh.acc : nullptr);
            if (own) { *own_first = lo; n_local = hi - lo; }
        }
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemsetAsync(sh.escaped, 0, sizeof(int), s));
        count_dirty = false;
        return push_counts(h, s);
    }
    // the own block's live bodies as records of `stride` bytes; *n_out = their number even when `cap` records are too few.
    // before_copy_out (may be null) runs after the synchronisation and before anything reaches the caller's buffer.
    int download_own(NbodyHandle* h, hipStream_t s, void* aos, size_t cap, size_t stride, size_t* n_out, int (*before_copy_out)(NbodyHandle*)) {
        int rc = sync_count(h, s);
        if (rc) return rc;
        const size_t n = n_local;
        if (n_out) *n_out = n;
        if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "download buffer too small");
        if (n == 0) return NBODY_OK;
        if (!aos) return fail(h, NBODY_ERR_INVALID, "null buffer");
        rc = ensure_aos(h, n);
        if (rc) return rc;
        nbody::launch_soa_to_aos<F>(s, d_aos, 10, int(n), sh.own_pos(), sh.vel, sh.acc);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(h_aos, d_aos, n * kRecBytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        if (before_copy_out) { rc = before_copy_out(h); if (rc) return rc; }
        char* dst = static_cast<char*>(aos);
        for (size_t k = 0; k < n; ++k) std::memcpy(dst + k * stride, h_aos + 10 * k, kRecBytes);
        return NBODY_OK;
    }
    // Vec::push (brute_force.rs:92-94) and Vec::swap_remove (brute_force.rs:96-98) on a world of one shard; both synchronise
    int push_one(NbodyHandle* h, hipStream_t s, const void* particle) {
        int rc = sync_count(h, s);
        if (rc) return rc;
        if (n_local >= size_t(sh.seg_cap)) return fail(h, NBODY_ERR_CAPACITY, "capacity exhausted");
        rc = ensure_aos(h, 1);
        if (rc) return rc;
        std::memcpy(h_aos, particle, kRecBytes);
        HIP_TRY(h, hipMemcpyAsync(d_aos, h_aos, kRecBytes, hipMemcpyHostToDevice, s));
        nbody::launch_aos_to_soa<F>(s, d_aos, 10, 1, sh.own_pos() + n_local, sh.vel + n_local, sh.acc + n_local);
        HIP_TRY(h, hipGetLastError());
        n_local += 1;
        seg_count_host[size_t(sh.my_seg)] = int(n_local);
        return push_own_count(h, s);
    }
    int swap_remove_one(NbodyHandle* h, hipStream_t s, size_t index) {
        int rc = sync_count(h, s);
        if (rc) return rc;
        if (index >= n_local) return fail(h, NBODY_ERR_INVALID, "swap_remove index out of range");  // Vec::swap_remove panics
        const size_t last = n_local - 1;
        if (index != last) {
            HIP_TRY(h, hipMemcpyAsync(sh.own_pos() + index, sh.own_pos() + last, sizeof(V4), hipMemcpyDeviceToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(sh.vel + index, sh.vel + last, sizeof(V4), hipMemcpyDeviceToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(sh.acc + index, sh.acc + last, sizeof(V4), hipMemcpyDeviceToDevice, s));
        }
        set_own_count(last);
        return push_own_count(h, s);
    }
    // the host's view after bodies were removed outside a step (swap_remove_one; nbody_merge_contacts, whose retain has
    // written the device's count already): exact
    void set_own_count(size_t n) {
        n_local = n;
        seg_count_host[size_t(sh.my_seg)] = int(n);
        count_dirty = false;
    }
};

// ---- the Barnes-Hut tree of a handle, for F = f32 and F = f64 (EngineBodies<F>::tree): the host build's
// tree, the node and order arrays the walks read, the device build's buffers, the walk's node-range split and the strict walk's
// stack, with the two procedures that fill them.  What walks the tree stays per precision (TreeDev, WalkSplit64 and their kernels).
template <class F> struct TreeTypes;
template <> struct TreeTypes<float> {
    using NodeDev = float4;               // 2 per node: {com, mass}, {width^2, skip, hot, leaf body}
    using StackEntry = float4;            // an open cell of k_bh_walk_nested
    static constexpr size_t kNodesPerBody = 4;   // the device build's first guess (a Plummer sphere gives ~1.5; the count read-back catches the rest)
};
template <> struct TreeTypes<double> {
    using NodeDev = nbody64::Node64;
    using StackEntry = nbody64::Open64;
    static constexpr size_t kNodesPerBody = 2;   // (64-byte records)
};

// what a build leaves for the walk that follows
struct TreeBuilt {
    bool fell_back = false;       // the device build met bodies deeper than it goes: the caller builds on the host
    int n_nodes = 0;
    const int* order = nullptr;   // device: own bodies (indices into the own segment) in tree order
    size_t n_order = 0;           // own bodies in the tree
    size_t n_tree = 0;            // bodies in the tree
};

template <class F>
struct TreeStore {
    using V4 = typename nbody::ShardT<F>::V4;
    using NodeDev = typename TreeTypes<F>::NodeDev;
    using StackEntry = typename TreeTypes<F>::StackEntry;
    static_assert(sizeof(nbody::NodeRecT<F>) == (sizeof(F) == 4 ? 2 : 1) * sizeof(NodeDev), "host and device node records must agree");

    nbody::HostTreeT<F> host;            // the last tree built on the host
    nbody::BuildScratchT<F> scratch;
    NodeDev* d_nodes = nullptr;          // one NodeRecT<F> per node
    int* d_order = nullptr;
    size_t node_cap = 0, order_cap = 0;  // nodes, ints
    F* h_pos = nullptr;                  // pinned: all segments' positions
    std::vector<int32_t> own_order;
    TreeBuildBufs bufs;                  // the device build's
    nbody::TreeDevWork work;             // arrays of the last device build (inside bufs.ws)
    bool on_device = false;              // the last tree was built on the device (export copies it back)
    size_t n_nodes = 0;                  // nodes of the last tree, wherever it was built
    WalkSplitBuf<V4> split;              // the walk's node-range split
    StackEntry* d_stack = nullptr;       // strict math, reference leaf rule: per-lane stack of open cells, [stack_levels][stack_lanes]
    size_t stack_lanes = 0;
    int stack_levels = 0;

    // a Barnes-Hut handle's host side: node arrays in pinned memory (their upload is one DMA) and the position mirror
    int alloc_host(NbodyHandle* h, const nbody::ShardT<F>& sh) {
        host.alloc = pinned_alloc;
        host.release = pinned_free;
        HIP_TRY(h, mem_of(h).pin(h_pos, size_t(sh.n_seg) * size_t(sh.seg_cap) * sizeof(V4)));
        return NBODY_OK;
    }
    int ensure_dev(NbodyHandle* h, size_t nodes, size_t order);   // grow-only (grow_dev)
    // the stack for trees of `levels` levels: one entry per open cell on a lane's path -- as many levels as the tree is deep
    // (the device build stops at 42; the host build reports its depth), not NBODY_MAX_TREE_DEPTH of them (13 GB at N = 2^22)
    int ensure_stack(NbodyHandle* h, int seg_cap, int levels);
    // The tree of a force pass built on the host (BarnesHutSimulation::update_forces, barnes_hut.rs:250-263): every block's
    // positions and live counts back with one synchronisation, build_octree<F>, the own bodies in tree order (ids are
    // block * seg_cap + index in the block), the nodes and that order up to the device.
    int build_on_host(NbodyHandle* h, BodyStore<F>& b, TreeBuilt* out);
    // The tree built on the device (kernels_tree.hip), over one shard or the concatenated index blocks: no positions go to the
    // host, no node array comes back; one read-back of {nodes, flags, bodies} and the blocks' live counts.  split (may be null):
    // the walk's split points ride in the build's last launch.  A node array that proves too small is grown once and rebuilt.
    int build_on_device(NbodyHandle* h, BodyStore<F>& b, bool want_hot, const nbody::TreeSplitReq* split_req, TreeBuilt* out);
    // com_mass [4 n] / width [n] / skip [n] (each may be null) of the last tree, fetched from the device when it lives there
    int export_nodes(NbodyHandle* h, F* com_mass, F* width, int32_t* skip, size_t cap, size_t* n_out);
};

// ---- what both engines keep per precision: nbody32::State and nbody64::State derive from it and keep the rest private to
// their translation units; every other unit reaches it through nbody32::bodies(h) / nbody64::bodies(h)
template <class F>
struct EngineBodies : BodyStore<F> {
    TreeStore<F> tree;           // Barnes-Hut: the tree, its device arrays, the device build's buffers, the walk's split and stack
    double* d_energy = nullptr;  // nbody_energy: per-block {KE, pair sum}
    size_t energy_blocks = 0;
};

// nbody_tracers_* (nbody_tracer.cpp): massless particles beside the bodies.  Their state is a second Shard of one segment, so
// the integrate and compact kernels run on it unchanged; n_host == 0 (no tracers) keeps every step path as it was.
struct TracerState {
    Shard sh;                    // pos (.w = 0), vel, acc, count, escape flag, keep flags, compaction words; the bodies' poison flag, no ids
    size_t cap = 0;              // tracers the arrays hold
    size_t n_host = 0;           // host view of the live count: exact after an upload or a read-back, an upper bound after a step
    bool dirty = false;          // a retain may have dropped tracers since n_host was read
    float4* d_planes = nullptr;  // [K][padded tracers] partial sums of the fast pass's body slices, grow-only
    size_t planes_cap = 0;       // float4 entries
    unsigned long long* d_stats = nullptr;   // [NBODY_WALK_COUNTER_SLOTS][2] directed interactions or accepted nodes, opening tests of the tracer passes
    // the tracer count at the upload: the fast passes' shapes are drawn from it (and the bodies' n_at_upload), not from
    // n_host / n_local, which a read-back refreshes
    size_t n_plan = 0;
    // Barnes-Hut handles: the tracers in tree order (keys and indices, unsorted | sorted), rocPRIM's scratch, the key kernel's info words
    unsigned long long* d_keys = nullptr;    // [2][sort_cap]
    int* d_idx = nullptr;                    // [2][sort_cap]
    void* d_sort_tmp = nullptr;
    int* d_info = nullptr;                   // [3]
    size_t sort_bytes = 0, sort_cap = 0;
};

// nbody_set_external_field (nbody_external.cpp): the components as given (f64); a pass rounds them to its precision.  n == 0 (no
// field) keeps every step path as it was.
struct ExternalField {
    int n = 0;
    NbodyExternalComponent given[NBODY_EXTERNAL_MAX] = {};
};

// nbody_set_mesh_gravity (nbody_mesh.cpp): the grid and the PM spec as given; on == false (never set, or cleared) keeps every
// step path as it was.  res: what stays on the device between passes, made by the first pass, freed on clear and on destroy.
namespace nbody { namespace mesh { struct Resident; } }
struct MeshGravity {
    bool on = false;
    NbodyGridSpec spec{};
    NbodyPmSpec pm{};
    nbody::mesh::Resident* res = nullptr;
    // nbody_mesh_gravity_stats: passes enqueued, the plan the last one used, 3-D transforms enqueued, allocations of the resident state
    uint64_t passes = 0, last_plan = 0, transforms = 0, allocations = 0;
};

// nbody_set_pair_search: how the fixed-radius calls find their pairs, and what the last of them left for
// nbody_pair_search_stats (nbody_cells.h).  Nothing else reads it.
struct PairSearch {
    int mode = NBODY_SEARCH_ALL_PAIRS;
    uint64_t last[4] = {0, 0, 0, 0};   // {ran the cell search, bodies gridded, occupied cells, candidate pairs}
};

struct NbodyHandle {
    nbody::HandleMem mem{kHipSeam};   // every device and pinned block of this handle, its f64 / spatial state included
    NbodyConfig cfg{};
    nbody::Tuning tune;        // this handle's launch-shape and scheme knobs (nbody_set_tuning; NBODY_* environment at create)
    int device = 0;
    hipStream_t stream = nullptr;
    ShardShape shape;          // the bodies themselves: f32 / f64 below
    size_t first_global = 0, n_at_upload = 0;   // the own index block at the last upload (both precisions)

    // Barnes-Hut
    std::unique_ptr<nbody::WorkerPool> pool;
    unsigned long long* d_counters = nullptr;  // [NBODY_WALK_COUNTER_SLOTS][2] accepted, visited (summed on read)
    // nbody_set_multipole: order of the force walk's expansion; 2 = the cells' quadrupole tensors beside the node records
    int multipole = NBODY_MULTIPOLE_MONOPOLE;
    float4* d_quad = nullptr;    // [quad_cap] records of kQuadRecBytes, in node order (kernels_quad.h)
    size_t quad_cap = 0;         // nodes
    bool quad_pass = false;      // the last force pass walked with quadrupoles (nbody_tree_export_quadrupoles)
    bool quad_call = false;      // the last tree was built by a call in NBODY_POTENTIAL_TREE_QUADRUPOLE (accepted by that export too)
    unsigned long long* h_counters = nullptr;  // pinned
    // Barnes-Hut steps enqueued without a read-back (nbody_f32.cpp State::async_bh): what a build that needs the host sets
    int* d_poison = nullptr;            // [2] sticky flags, steps completed (Shard::poison)
    int* h_poison = nullptr;            // pinned [8]: poison[2] + tree info[3]; between their own synchronisations also scratch, at the offsets below

    // diagnostics
    NbodyStats stats{};
    bool profiling = false;
    int profile_every = 1;       // bracket every k-th force-kernel launch with events (nbody_set_profiling(h, k))
    unsigned profile_tick = 0;
    bool timed_this = false;     // the launch under way is one of the bracketed ones
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending, ev_free;
    PotBufs pot;
    FieldBufs field;
    TracerState tr;
    ExternalField ext;
    MeshGravity mesh;
    PairSearch search;
    uint64_t deposit_last[4] = {0, 0, 0, 0};   // nbody_deposit_stats: {a call reached the device, its plan, terms on the grid, global atomics}
    uint64_t poisson_last[4] = {0, 0, 0, 0};   // nbody_grid_poisson_stats: {a call reached the device, the plan it used, butterfly launches, complex points transformed}
    uint64_t sample_last[4] = {0, 0, 0, 0};    // nbody_grid_sample_stats: {a call reached the device, the plan it used, grid reads of k_sample, 0}
    uint64_t pm_last[4] = {0, 0, 0, 0};        // nbody_pm_field_stats: {a call reached the device, the plan it used, grid reads of the gather, radix sorts enqueued}
    uint64_t p3m_last[4] = {0, 0, 0, 0};       // nbody_p3m_field_stats: {a call reached the device, the plan it used, partners looked at, terms with r2 < R2}

    // multi-GPU: what carries the exchanges (RCCL, or the one-device transport of transport_ipc.hip)
    std::unique_ptr<nbody::Transport> tp;
    bool comm_ready = false;
    hipStream_t comm_stream = nullptr;   // the exchange runs here, beside the own-shard force kernel
    hipEvent_t ev_drifted = nullptr, ev_gathered = nullptr;
    bool exchange_in_flight = false;

    // the engine of the handle's precision: its EngineBodies<F> and what it keeps beside them, private to its translation unit
    nbody32::State* f32 = nullptr;   // NbodyConfig.dtype == NBODY_F32
    nbody64::State* f64 = nullptr;   // NbodyConfig.dtype == NBODY_F64
    nbody::let::State* let = nullptr; // NbodyConfig.shard_mode == NBODY_SHARD_SPATIAL (beside f32): the halo-exchange machinery

    std::string err;
};


// ---- helpers that need the handle

// NbodyHandle::h_poison as pinned scratch for small read-backs: each user copies, synchronises and reads at once
constexpr int kScratchStats = 4;          // one u64 ([4..5]): nbody_stats' interaction count
constexpr int kScratchTracerCount = 6;    // one int: the live tracer count, up and down

inline nbody::HandleMem& mem_of(NbodyHandle* h) { return h->mem; }

// grow-only device array: to grow_cap(rule, n) elements of elem_bytes when it holds fewer than n (HandleMem::grow: a failure
// leaves p null and cap 0).  kGrowSync: the stream is synchronised before the old block goes (something enqueued may still
// read it); kGrowZero: the new block is zeroed on the stream.  For HIP_TRY.
enum { kGrowSync = 1, kGrowZero = 2 };
template <class T>
hipError_t grow_dev(NbodyHandle* h, T*& p, size_t& cap, size_t n, size_t elem_bytes, Grow rule, int how = 0) {
    if (n <= cap) return hipSuccess;
    if ((how & kGrowSync) && p) {
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return e;
    }
    const int e = h->mem.grow(p, cap, n, elem_bytes, rule);
    if (e) return hipError_t(e);
    return (how & kGrowZero) ? hipMemsetAsync(p, 0, cap * elem_bytes, h->stream) : hipSuccess;
}
// ... keeping the first `keep` elements (HandleMem::grow_keep); the stream is synchronised before the old block goes
template <class T>
hipError_t grow_dev_keep(NbodyHandle* h, T*& p, size_t& cap, size_t n, size_t elem_bytes, Grow rule, size_t keep) {
    return hipError_t(h->mem.grow_keep(p, cap, n, elem_bytes, rule, keep, [h](void* fresh, const void* old, size_t bytes) {
        hipError_t e = bytes ? hipMemcpyAsync(fresh, old, bytes, hipMemcpyDeviceToDevice, h->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        return int(e);
    }));
}

// The live rows of sh: the device's count word copied and waited for, clamped to [0, n_upper] (the host's view of the count is
// left as it is), for the calls that must know how many rows they will return before they write anything.
template <class S>
hipError_t live_rows(NbodyHandle* h, const S& sh, size_t n_upper, size_t* live) {
    int n_live = 0;
    hipError_t e = hipSuccess;
    if (n_upper) {
        e = hipMemcpyAsync(&n_live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
        const hipError_t e_sync = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = e_sync;
    }
    *live = e == hipSuccess ? std::min(size_t(std::max(n_live, 0)), n_upper) : 0;
    return e;
}

// what follows it in a call that returns one row per live body; *n_out (may be null) is set even when the buffer is too small
inline int row_frame(NbodyHandle* h, const char* call, const char* buffer, size_t live, const void* out, size_t cap, size_t* n_out) {
    if (live && !out) return fail(h, NBODY_ERR_INVALID, std::string(call) + ": " + buffer + " is NULL");
    if (n_out) *n_out = live;
    if (live > cap) return fail(h, NBODY_ERR_CAPACITY, std::string(call) + ": buffer too small");
    return NBODY_OK;
}

// What a grid call (deposit, sample, Poisson, PM field, mesh pass) has enqueued on the handle's stream, as one status: a HIP error
// or a rocPRIM call that could not be enqueued.  Once it is not ok() the caller enqueues nothing more: `if (st.ok()) st.hip(...)`.
class Enqueued {
public:
    bool ok() const { return e_ == hipSuccess && !prim_failed_; }
    void hip(hipError_t e) { if (ok()) e_ = e; }                // the first failure is kept
    void prim(int rc) { if (ok() && rc != 0) prim_failed_ = true; }   // rc: a launcher's 0 or -1
    void last() { if (e_ == hipSuccess) e_ = hipGetLastError(); }     // a launch that failed, asked for even after a rocPRIM failure
    // nothing waited for: the HIP error first, then the rocPRIM failure under the call's name, then NBODY_OK
    int result(NbodyHandle* h, const char* call) const {
        const hipError_t e = e_;
        HIP_TRY(h, e);
        if (prim_failed_) return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
        return NBODY_OK;
    }
    // The end of a call that waits: the stream is synchronised ALWAYS, whatever was enqueued and whether or not it failed.  The
    // copies write the caller's locals and the user's buffers and read host tables of the caller's frame, and the scratch goes
    // with the frame or is reused by the next batch: none may go out of reach while anything on the stream can touch it.
    int finish(NbodyHandle* h, const char* call) {
        const hipError_t e_sync = hipStreamSynchronize(h->stream);
        if (e_ == hipSuccess) e_ = e_sync;
        return result(h, call);
    }
private:
    hipError_t e_ = hipSuccess;   // the first that was not hipSuccess
    bool prim_failed_ = false;
};

struct ForceTimer {  // HIP events around a force-kernel launch, on the launch stream
    NbodyHandle* h;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    explicit ForceTimer(NbodyHandle* hh) : h(hh) {
        h->timed_this = false;
        if (!h->profiling) return;
        // (an event pair costs the stream ~11 us: with nbody_set_profiling(h, k > 1) only every k-th launch is bracketed)
        if (h->profile_every > 1 && (h->profile_tick++ % unsigned(h->profile_every)) != 0) return;
        h->timed_this = true;
        if (!h->ev_free.empty()) { ev = h->ev_free.back(); h->ev_free.pop_back(); }
        else {
            if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) { ev = {nullptr, nullptr}; return; }
        }
        (void)hipEventRecord(ev.first, h->stream);
    }
    ~ForceTimer() {
        if (!ev.first) return;
        (void)hipEventRecord(ev.second, h->stream);
        h->ev_pending.push_back(ev);
    }
};
// folds the bracketed launches' timings into the statistics (synchronises when there are any)
inline int drain_events(NbodyHandle* h) {
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

// ---- TreeStore<F>'s procedures (they need the handle: its stream, worker pool and statistics)

template <class F>
int TreeStore<F>::ensure_dev(NbodyHandle* h, size_t nodes, size_t order) {
    HIP_TRY(h, grow_dev(h, d_nodes, node_cap, nodes, sizeof(nbody::NodeRecT<F>), Grow::quarter));
    HIP_TRY(h, grow_dev(h, d_order, order_cap, order, sizeof(int), Grow::quarter));
    return NBODY_OK;
}

template <class F>
int TreeStore<F>::ensure_stack(NbodyHandle* h, int seg_cap, int levels) {
    const size_t lanes = (size_t(seg_cap) + 255) / 256 * 256;
    if (lanes > stack_lanes || levels > stack_levels) {   // (a cap of two dimensions: the block replaces its old one)
        stack_lanes = 0; stack_levels = 0;
        const int lv = std::max(levels + 8, 32);
        HIP_TRY(h, h->mem.dev(d_stack, lanes * size_t(lv) * sizeof(StackEntry)));
        stack_lanes = lanes; stack_levels = lv;
    }
    return NBODY_OK;
}

template <class F>
int TreeStore<F>::build_on_host(NbodyHandle* h, BodyStore<F>& b, TreeBuilt* out) {
    const nbody::ShardT<F>& sh = b.sh;
    const int n_seg = sh.n_seg, seg_cap = sh.seg_cap;
    const F* pos_all = reinterpret_cast<const F*>(sh.pos_all);
    on_device = false;
    auto t0 = clk::now();
    for (int g = 0; g < n_seg; ++g) {
        const size_t cnt = size_t(b.seg_count_host[size_t(g)]);
        if (cnt)
            HIP_TRY(h, hipMemcpyAsync(h_pos + 4 * size_t(g) * seg_cap, pos_all + 4 * size_t(g) * seg_cap, cnt * 4 * sizeof(F),
                                      hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(b.h_counts, sh.seg_count, sizeof(int) * n_seg, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int g = 0; g < n_seg; ++g) b.seg_count_host[size_t(g)] = b.h_counts[g];
    b.n_local = size_t(b.h_counts[sh.my_seg]);
    b.count_dirty = false;
    const double copy_ms = ms_since(t0);

    auto t1 = clk::now();
    nbody::build_octree<F>(h_pos, n_seg, seg_cap, b.h_counts, b.center, b.width, *h->pool, scratch, host);
    n_nodes = host.n_nodes;
    if (host.too_deep) return fail(h, NBODY_ERR_TREE_DEPTH, "octree deeper than NBODY_MAX_TREE_DEPTH (coincident bodies?)");
    const int32_t* order = host.order;
    size_t n_order = host.n_order;
    if (n_seg > 1) {
        own_order.clear();
        const int lo = sh.my_seg * seg_cap, hi = lo + seg_cap;
        for (size_t k = 0; k < host.n_order; ++k) {
            const int id = host.order[k];
            if (id >= lo && id < hi) own_order.push_back(id - lo);
        }
        order = own_order.data();
        n_order = own_order.size();
    }
    h->stats.tree_build_ms += ms_since(t1);
    h->stats.tree_nodes = host.n_nodes;

    auto t2 = clk::now();
    int rc = ensure_dev(h, host.n_nodes, n_order);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(d_nodes, host.nodes, host.n_nodes * sizeof(nbody::NodeRecT<F>), hipMemcpyHostToDevice, h->stream));
    if (n_order) HIP_TRY(h, hipMemcpyAsync(d_order, order, n_order * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (n_seg > 1) HIP_TRY(h, hipStreamSynchronize(h->stream));   // own_order is pageable and reused
    h->stats.tree_copy_ms += copy_ms + ms_since(t2);
    *out = TreeBuilt{false, int(host.n_nodes), d_order, n_order, host.n_order};
    return NBODY_OK;
}

template <class F>
int TreeStore<F>::build_on_device(NbodyHandle* h, BodyStore<F>& b, bool want_hot, const nbody::TreeSplitReq* split_req, TreeBuilt* out) {
    const nbody::ShardT<F>& sh = b.sh;
    *out = TreeBuilt{};
    auto t0 = clk::now();
    const bool sharded = sh.n_seg > 1;   // every GPU builds the same tree over the gathered bodies of all segments
    const size_t n_cap = size_t(sh.seg_cap) * size_t(sh.n_seg);
    int rc = bufs.ensure(h, n_cap, sharded ? nbody::tree_cat_bytes<V4>(n_cap) : 0);
    if (rc) return rc;
    size_t tot_upper = b.n_local;
    if (sharded) { tot_upper = 0; for (int c : b.seg_count_host) tot_upper += size_t(c); }
    rc = ensure_dev(h, TreeTypes<F>::kNodesPerBody * tot_upper + 64, tot_upper);
    if (rc) return rc;
    nbody::TreeCat<V4> cat;
    const V4* tree_pos = sh.own_pos();
    const int* tree_count = sh.own_count();
    if (sharded) {
        cat = nbody::tree_cat_layout<V4>(bufs.cat, n_cap);
        nbody::launch_tree_cat(h->stream, sh, cat);
        tree_pos = cat.pos;
        tree_count = cat.info;
    }
    for (int attempt = 0;; ++attempt) {
        if (nbody::build_octree_device(h->stream, tree_pos, tree_count, int(tot_upper), b.center, b.width, bufs.ws, n_cap, d_nodes,
                                       int(std::min<size_t>(node_cap, 0x7fffffff)), d_order, bufs.d_info, &work, want_hot ? 1 : 0, split_req) != 0)
            return fail(h, NBODY_ERR_HIP, "device octree build: rocPRIM call failed");
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(bufs.h_info, bufs.d_info, 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (sharded) HIP_TRY(h, hipMemcpyAsync(b.h_counts, sh.seg_count, sizeof(int) * sh.n_seg, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (!sharded) b.h_counts[0] = bufs.h_info[2];   // one shard: the tree's body count is the live count
        if (!(bufs.h_info[1] & 2) || (bufs.h_info[1] & 5)) break;
        if (attempt == 1) return fail(h, NBODY_ERR_CAPACITY, "device octree build: node array too small twice");
        rc = ensure_dev(h, size_t(bufs.h_info[0]) + 64, tot_upper);   // more nodes than allowed for: the build says how many; grow, rebuild
        if (rc) return rc;
    }
    size_t n_tree = 0;
    for (int g = 0; g < sh.n_seg; ++g) { b.seg_count_host[size_t(g)] = b.h_counts[g]; n_tree += size_t(b.h_counts[g]); }
    b.n_local = size_t(b.h_counts[sh.my_seg]);
    b.count_dirty = false;
    if (bufs.h_info[1] & 5) { out->fell_back = true; return NBODY_OK; }   // deeper than 42 levels / a clump beyond the build's sort
    const int* order = d_order;
    if (sharded) {   // the own bodies' places in the tree order
        if (nbody::launch_tree_own_order(h->stream, d_order, cat, int(n_tree), bufs.ws, nbody::tree_build_tmp_bytes(n_cap)) != 0)
            return fail(h, NBODY_ERR_HIP, "device octree build: rocPRIM call failed");
        order = cat.own_order;
    }
    on_device = true;
    n_nodes = size_t(bufs.h_info[0]);
    h->stats.tree_build_ms += ms_since(t0);
    h->stats.tree_nodes = n_nodes;
    *out = TreeBuilt{false, bufs.h_info[0], order, b.n_local, n_tree};
    return NBODY_OK;
}

template <class F>
int TreeStore<F>::export_nodes(NbodyHandle* h, F* com_mass, F* width, int32_t* skip, size_t cap, size_t* n_out) {
    const size_t n = n_nodes;
    if (n_out) *n_out = n;
    if (!com_mass && !width && !skip) return NBODY_OK;
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "tree export buffer too small");
    std::vector<nbody::NodeRecT<F>> from_device;
    if (on_device) {   // the octree lives on the device only: fetch it
        from_device.resize(n);
        if (n) HIP_TRY(h, hipMemcpyAsync(from_device.data(), d_nodes, n * sizeof(nbody::NodeRecT<F>), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    const nbody::NodeRecT<F>* nodes = on_device ? from_device.data() : host.nodes;
    for (size_t i = 0; i < n; ++i) {
        const nbody::NodeRecT<F>& r = nodes[i];
        if (com_mass) { com_mass[4 * i] = r.a.x; com_mass[4 * i + 1] = r.a.y; com_mass[4 * i + 2] = r.a.z; com_mass[4 * i + 3] = r.a.m; }
        if (width) width[i] = std::sqrt(r.b.w2);  // exact: w2 is the rounded square of the width
        if (skip) skip[i] = r.b.skip;
    }
    return NBODY_OK;
}
