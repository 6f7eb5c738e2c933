// nbody_pm.cpp -- nbody_pm_field and nbody_pm_field_at (include/nbody_hip.h, "particle-mesh field"): the one scratch of a call,
// the launches of the deposit, the Poisson solve and the gather against the grid that stays on the device, the copies of the
// rows, the classes and the words, and the one synchronisation.  The host twin is pm_grid.h's.
#include "nbody_pm.h"

#include "nbody_poisson.h"   // enqueue
#include "nbody_sample.h"    // kPointBatch

#include <algorithm>
#include <string>

namespace nbody { namespace pm {

namespace {

// what one pass over rows brings down
struct Down {
    deposit::Words dep{};
    sample::Words rows{}, value{};
};

}  // namespace

// (the contracts of enqueue_grid and enqueue_rows are nbody_pm.h's)
template <class F>
hipError_t enqueue_grid(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, const Call& c,
                        const Scratch& w, const int* ordered_rows, bool* sort_failed, uint64_t* sorts, int held, uint64_t* transforms) {
    const hipStream_t s = h->stream;
    if (n_upper) {
        deposit::launch_q<F>(s, sh, int(n_upper), c.g, NBODY_DEPOSIT_MASS, w.dep);
        if (deposit::launch_deposit<F>(s, sh, int(n_upper), c.g, c.plans.dep, w.dep, ordered_rows) != 0) {
            *sort_failed = true;
            return hipSuccess;
        }
        if (c.plans.dep.sort && !ordered_rows) ++*sorts;
    } else {   // no body: every count 0 and every cell +0.0
        (void)hipMemsetAsync(w.dep.words, 0, sizeof(deposit::Words), s);
        (void)hipMemsetAsync(w.dep.acc, 0, deposit::cells_of(c.g) * sizeof(long long), s);
    }
    hipError_t e = hipGetLastError();
    int made = 0;
    if (e == hipSuccess) e = poisson::enqueue(h, spec, pm.poisson, c.shape, c.tables, c.plans.poi, w.poi, nullptr, &made, held);
    if (e == hipSuccess && transforms) *transforms += uint64_t(made);
    if (e == hipSuccess && c.plans.grad.pregrad) {
        sample::launch_diff(s, c.g, c.op, w.smp);
        e = hipGetLastError();
    }
    return e;
}

int enqueue_rows(NbodyHandle* h, const Call& c, const int* count, size_t n, bool with_phi, bool ordered, const Scratch& w, uint64_t* sorts) {
    const hipStream_t s = h->stream;
    const Plans& p = c.plans;
    if (p.grad.sort && !ordered) {
        if (sample::launch_order(s, count, int(n), c.g, w.smp) != 0) return -1;
        ++*sorts;
    }
    if (p.pm.gather) {
        launch_gather(s, count, int(n), c.g, c.op, with_phi, p.grad.sort ? w.smp.rows + n : nullptr, w);
        return 0;
    }
    // the cross-check: k_sample twice over the same order, gradient then value
    (void)sample::launch_sample(s, count, int(n), c.g, 1, c.op, p.grad, w.smp, true);
    launch_negate(s, count, int(n), w.smp.out);
    sample::Scratch v = w.smp;
    v.out = w.phi;
    v.cls = w.value_cls;
    v.words = w.value_words;
    if (with_phi) (void)sample::launch_sample(s, count, int(n), c.g, 1, NBODY_SAMPLE_VALUE, p.value, v, true);
    else (void)hipMemsetAsync(v.words, 0, sizeof(sample::Words), s);
    return 0;
}

namespace {

// the copies of a pass's first `copy` rows and of its words, enqueued (e: what went before; nothing more once it failed)
hipError_t enqueue_down(NbodyHandle* h, hipError_t e, const Call& c, const Scratch& w, size_t copy, double* acc, double* phi, uint8_t* cls,
                        Down* down) {
    const hipStream_t s = h->stream;
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&down->rows, w.smp.words, sizeof(sample::Words), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !c.plans.pm.gather) e = hipMemcpyAsync(&down->value, w.value_words, sizeof(sample::Words), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && copy) e = hipMemcpyAsync(acc, w.smp.out, copy * 3 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && copy && phi) e = hipMemcpyAsync(phi, w.phi, copy * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && copy && cls) e = hipMemcpyAsync(cls, w.smp.cls, copy, hipMemcpyDeviceToHost, s);
    return e;
}

void record(NbodyHandle* h, const Call& c, uint64_t reads, uint64_t sorts) {
    h->pm_last[0] = 1;
    h->pm_last[1] = uint64_t(c.plans.pm.gather | (c.plans.shared ? 2 : 0));
    h->pm_last[2] = reads;
    h->pm_last[3] = sorts;
}

}  // namespace

template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, double* acc, double* phi,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts) {
    // the live count first: a call that is refused, a buffer that is too small included, computes and writes nothing
    int n_live = 0;
    if (n_upper) {
        const hipError_t e = hipMemcpyAsync(&n_live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
        const hipError_t e_sync = hipStreamSynchronize(h->stream);
        HIP_TRY(h, e);
        HIP_TRY(h, e_sync);
    }
    const size_t live = std::min(size_t(std::max(n_live, 0)), n_upper);
    if (live && !acc) return fail(h, NBODY_ERR_INVALID, "nbody_pm_field: acc is NULL");
    if (n_out) *n_out = live;
    if (live > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_pm_field: buffer too small");
    if (counts) std::fill(counts, counts + 8, uint64_t(0));
    if (!live) return NBODY_OK;
    const Call c(spec, pm, true);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, n_upper, c.g, c.shape, c.deconvolve, c.op, c.plans)));
    const Scratch w = scratch_layout(scratch.get(), n_upper, n_upper, c.g, c.shape, c.deconvolve, c.op, c.plans);
    const hipStream_t s = h->stream;
    uint64_t sorts = 0;
    bool sort_failed = false;
    sample::launch_stage<F>(s, sh, int(n_upper), w.smp);
    const int* order = nullptr;   // one order for both stages: the sampler's keys, which depend on the position alone
    if (c.plans.shared) {
        sort_failed = sample::launch_order(s, sh.own_count(), int(n_upper), c.g, w.smp) != 0;
        order = w.smp.rows + n_upper;
        ++sorts;
    }
    hipError_t e = hipSuccess;
    if (!sort_failed) e = enqueue_grid<F>(h, sh, n_upper, spec, pm, c, w, order, &sort_failed, &sorts);
    if (e == hipSuccess && !sort_failed) sort_failed = enqueue_rows(h, c, sh.own_count(), n_upper, phi != nullptr, c.plans.shared, w, &sorts) != 0;
    // (down is a local, the tables are c's and the rows the user's: whatever was enqueued is waited for before any goes out of reach)
    Down down;
    if (e == hipSuccess && !sort_failed) e = hipMemcpyAsync(&down.dep, w.dep.words, sizeof(deposit::Words), hipMemcpyDeviceToHost, s);
    if (!sort_failed) e = enqueue_down(h, e, c, w, live, acc, phi, cls, &down);
    const hipError_t e_sync = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e_sync;
    HIP_TRY(h, e);
    if (sort_failed) return fail(h, NBODY_ERR_HIP, "nbody_pm_field: rocPRIM call failed");
    if (counts) {
        std::copy(down.dep.counts, down.dep.counts + 4, counts);
        std::copy(down.rows.counts, down.rows.counts + 4, counts + 4);
    }
    record(h, c, down.rows.reads + down.value.reads, sorts);
    return NBODY_OK;
}

template <class F>
int at_points(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, const double* xyz,
              size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts) {
    if (counts) std::fill(counts, counts + 8, uint64_t(0));
    const Call c(spec, pm, false);
    const size_t batch = std::max<size_t>(std::min(n_points, sample::kPointBatch), 1);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, batch, c.g, c.shape, c.deconvolve, c.op, c.plans)));
    const Scratch w = scratch_layout(scratch.get(), n_upper, batch, c.g, c.shape, c.deconvolve, c.op, c.plans);
    const hipStream_t s = h->stream;
    uint64_t sorts = 0, reads = 0, counted[4] = {0, 0, 0, 0};
    bool sort_failed = false;
    Down down;
    hipError_t e = enqueue_grid<F>(h, sh, n_upper, spec, pm, c, w, nullptr, &sort_failed, &sorts);
    if (e == hipSuccess && !sort_failed) e = hipMemcpyAsync(&down.dep, w.dep.words, sizeof(deposit::Words), hipMemcpyDeviceToHost, s);
    // (every pass ends in a synchronisation, whatever was enqueued: the batch's buffers are reused by the next one, and down, the
    // tables and the user's rows must not go out of reach before)
    size_t at0 = 0;
    do {
        const size_t n = std::min(batch, n_points - at0);
        if (e == hipSuccess && !sort_failed && n) {
            e = hipMemcpyAsync(w.smp.xyz, xyz + 3 * at0, n * 3 * sizeof(double), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) sort_failed = enqueue_rows(h, c, nullptr, n, phi != nullptr, false, w, &sorts) != 0;
            if (!sort_failed) e = enqueue_down(h, e, c, w, n, acc + 3 * at0, phi ? phi + at0 : nullptr, cls ? cls + at0 : nullptr, &down);
        }
        const hipError_t e_sync = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e_sync;
        HIP_TRY(h, e);
        if (sort_failed) return fail(h, NBODY_ERR_HIP, "nbody_pm_field_at: rocPRIM call failed");
        for (int k = 0; k < 4; ++k) counted[k] += down.rows.counts[k];
        reads += down.rows.reads + down.value.reads;
        down.rows = sample::Words{};
        down.value = sample::Words{};
        at0 += n;
    } while (at0 < n_points);
    if (counts) {
        std::copy(down.dep.counts, down.dep.counts + 4, counts);
        std::copy(counted, counted + 4, counts + 4);
    }
    record(h, c, reads, sorts);
    return NBODY_OK;
}

template hipError_t enqueue_grid<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const Call&, const Scratch&,
                                        const int*, bool*, uint64_t*, int, uint64_t*);
template hipError_t enqueue_grid<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const Call&, const Scratch&,
                                         const int*, bool*, uint64_t*, int, uint64_t*);
template int at_bodies<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, double*, double*, uint8_t*,
                              size_t, size_t*, uint64_t*);
template int at_bodies<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, double*, double*, uint8_t*,
                               size_t, size_t*, uint64_t*);
template int at_points<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const double*, size_t, double*,
                              double*, uint8_t*, uint64_t*);
template int at_points<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const double*, size_t, double*,
                               double*, uint8_t*, uint64_t*);

}}  // namespace nbody::pm
