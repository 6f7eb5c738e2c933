// nbody_engine.h -- the one way from a handle to the bodies of its precision (with_bodies), and what nbody_f32.cpp and
// nbody_f64.cpp would otherwise each spell out: the host calls that are the same text up to F, once, over EngineBodies<F>.
// Each engine's entry point stays a wrapper that adds what is its own (resolve_async first, the Hermite flags after).
#pragma once
#include "nbody_f32.h"
#include "nbody_f64.h"
#include "nbody_pot.h"

// fn(EngineBodies<float>&) on an f32 handle, fn(EngineBodies<double>&) on an f64 one (const stores for a const handle); both
// must return the same type.  Settings read through it come from the store that holds them, to be widened by the reader.
template <class H, class Fn>
auto with_bodies(H* h, Fn&& fn) { return h->f64 ? fn(nbody64::bodies(h)) : fn(nbody32::bodies(h)); }

namespace engine {

using nbody::launch_energy;
using nbody64::launch_energy;

// the host's view of the world's body count (an upper bound while count_dirty)
template <class F>
size_t total_upper(const BodyStore<F>& b) {
    size_t t = 0;
    for (int c : b.seg_count_host) t += size_t(c);
    return t;
}

template <class F>
int upload(NbodyHandle* h, BodyStore<F>& b, const void* aos, size_t n, size_t stride) {
    const int rc = b.upload_blocks(h, h->stream, aos, n, stride, &h->first_global);
    h->n_at_upload = b.n_local;
    return rc;
}

template <class F>
int count(NbodyHandle* h, BodyStore<F>& b, size_t* n_out) {
    const int rc = b.sync_count(h, h->stream);
    if (!rc) *n_out = b.n_local;
    return rc;
}

template <class F>
int count_global(NbodyHandle* h, BodyStore<F>& b, size_t* n_out) {   // as of the last exchange
    const int rc = b.sync_count(h, h->stream);
    if (!rc) *n_out = total_upper(b);
    return rc;
}

template <class F>
int stats(NbodyHandle* h, const BodyStore<F>& b, NbodyStats* out) {
    if (h->cfg.method == NBODY_BRUTE_FORCE) {   // (NbodyStats::interactions is counted on the device from the live counts: Shard::inter)
        unsigned long long* hv = reinterpret_cast<unsigned long long*>(h->h_poison + kScratchStats);
        HIP_TRY(h, hipMemcpyAsync(hv, b.sh.inter, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
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

template <class F>
int reset_stats(NbodyHandle* h, BodyStore<F>& b) {
    HIP_TRY(h, hipMemsetAsync(b.sh.inter, 0, sizeof(unsigned long long), h->stream));
    return NBODY_OK;
}

// nbody_energy: KE and the pair sum over the own block, block partials added in block order
template <class F>
int energy(NbodyHandle* h, EngineBodies<F>& b, double* kinetic, double* potential) {
    int rc = b.sync_count(h, h->stream);
    if (rc) return rc;
    const size_t n = b.n_local;
    const size_t blocks = (n + 255) / 256;
    double ke = 0.0, pe = 0.0;
    if (blocks) {
        HIP_TRY(h, grow_dev(h, b.d_energy, b.energy_blocks, blocks, 2 * sizeof(double), Grow::exact));
        launch_energy(h->stream, b.sh, int(n), double(b.g_soft) * double(b.g_soft), b.d_energy);
        HIP_TRY(h, hipGetLastError());
        std::vector<double> part(blocks * 2);
        HIP_TRY(h, hipMemcpyAsync(part.data(), b.d_energy, blocks * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < blocks; ++k) { ke += part[2 * k]; pe += part[2 * k + 1]; }
    }
    if (kinetic) *kinetic = ke;
    if (potential) *potential = -0.5 * double(b.g) * pe;  // every unordered pair was met twice
    return NBODY_OK;
}

// index-block shards: every block's positions and live count into every rank's pos_all / seg_count, in place, as one group on
// `on`
template <class F>
int gather_blocks(NbodyHandle* h, BodyStore<F>& b, hipStream_t on) {
    if (!h->comm_ready) return fail(h, NBODY_ERR_COMM, "world_size > 1 but nbody_comm_init has not been called");
    TP_TRY(h, h->tp->group_begin());
    TP_TRY(h, h->tp->all_gather(b.sh.pos_all, size_t(b.sh.seg_cap) * sizeof(typename BodyStore<F>::V4), on));
    TP_TRY(h, h->tp->all_gather(b.sh.seg_count, sizeof(int), on));
    TP_TRY(h, h->tp->group_end());
    return NBODY_OK;
}

// What potentials_device does to the host's view of the counts, for the lifetime of this object: begin() makes them exact
// (the call reports and sums over live bodies), the destructor puts the view back as it was -- a step chain enqueued without
// read-back sizes its launches from the bound it has, and must do so with or without the call.
template <class F>
struct PotView {
    BodyStore<F>& b;
    const size_t n_local;
    const bool count_dirty;
    const std::vector<int> seg_count_host;
    explicit PotView(BodyStore<F>& bb) : b(bb), n_local(bb.n_local), count_dirty(bb.count_dirty), seg_count_host(bb.seg_count_host) {}
    ~PotView() { b.n_local = n_local; b.count_dirty = count_dirty; b.seg_count_host = seg_count_host; }
    PotView(const PotView&) = delete;
    PotView& operator=(const PotView&) = delete;
    // + PotBufs for the call (pot::begin), the bodies as the pair and energy kernels see them, the store's g
    int begin(NbodyHandle* h, nbody::PotBodies* bodies, double* g) {
        b.count_dirty = true;
        int rc = b.sync_count(h, h->stream);
        if (!rc) rc = nbody::pot::begin(h, size_t(b.sh.seg_cap));
        bodies->pos_all = b.sh.pos_all; bodies->vel = b.sh.vel; bodies->seg_count = b.sh.seg_count;
        bodies->f64 = sizeof(F) == sizeof(double); bodies->n_seg = b.sh.n_seg; bodies->seg_cap = b.sh.seg_cap; bodies->my_seg = b.sh.my_seg;
        bodies->world = b.sh.n_seg;
        *g = double(b.g);
        return rc;
    }
};

}  // namespace engine
