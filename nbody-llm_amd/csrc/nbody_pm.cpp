// nbody_pm.cpp -- nbody_pm_field and nbody_pm_field_at (include/nbody_hip.h, "particle-mesh field"): the one scratch of a call,
// the launches of the deposit, the Poisson solve and the gather against the grid that stays on the device, the copies of the
// rows, the classes and the words, and the one synchronisation.  The host twin is pm_grid.h's.
#include "nbody_pm.h"

#include "nbody_poisson.h"   // enqueue
#include "nbody_sample.h"    // kPointBatch

#include <algorithm>
#include <string>

namespace nbody { namespace pm {

// (the contracts of the stages are nbody_pm.h's)
const int* enqueue_shared_order(NbodyHandle* h, const Call& c, const int* count, size_t n, bool shared, const Scratch& w, Enqueued& st, Tally& tally) {
    if (!shared) return nullptr;
    st.prim(sample::launch_order(h->stream, count, int(n), c.g, w.smp));
    ++tally.sorts;
    return w.smp.rows + n;
}

template <class F>
void enqueue_grid(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, const Call& c,
                  const Scratch& w, const int* ordered_rows, Enqueued& st, Tally& tally, int held) {
    const hipStream_t s = h->stream;
    if (!st.ok()) return;
    if (n_upper) {
        deposit::launch_q<F>(s, sh, int(n_upper), c.g, NBODY_DEPOSIT_MASS, w.dep);
        st.prim(deposit::launch_deposit<F>(s, sh, int(n_upper), c.g, c.plans.dep, w.dep, ordered_rows));
        if (!st.ok()) return;
        if (c.plans.dep.sort && !ordered_rows) ++tally.sorts;
    } else {   // no body: every count 0 and every cell +0.0
        (void)hipMemsetAsync(w.dep.words, 0, sizeof(deposit::Words), s);
        (void)hipMemsetAsync(w.dep.acc, 0, deposit::cells_of(c.g) * sizeof(long long), s);
    }
    st.last();
    int made = 0;
    if (st.ok()) st.hip(poisson::enqueue(h, spec, pm.poisson, c.shape, c.tables, c.plans.poi, w.poi, nullptr, &made, held, c.split));
    if (st.ok()) tally.transforms += uint64_t(made);
    if (st.ok() && c.plans.grad.pregrad) {
        sample::launch_diff(s, c.g, c.op, w.smp);
        st.last();
    }
}

void enqueue_rows(NbodyHandle* h, const Call& c, const int* count, size_t n, bool with_phi, bool ordered, const Scratch& w, Enqueued& st, Tally& tally) {
    const hipStream_t s = h->stream;
    const Plans& p = c.plans;
    if (!st.ok()) return;
    int rc = 0;
    const int* rows = sample::ordered_rows(s, count, int(n), c.g, w.smp, p.grad.sort != 0, ordered, &rc, &tally.sorts);
    st.prim(rc);
    if (!st.ok()) return;
    if (p.pm.gather) {
        launch_gather(s, count, int(n), c.g, c.op, with_phi, rows, w);
        return;
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
}

void enqueue_down(NbodyHandle* h, Enqueued& st, const Call& c, const Scratch& w, size_t copy, double* acc, double* phi, uint8_t* cls, Down* down) {
    const hipStream_t s = h->stream;
    if (st.ok()) st.last();
    if (st.ok()) st.hip(hipMemcpyAsync(&down->rows, w.smp.words, sizeof(sample::Words), hipMemcpyDeviceToHost, s));
    if (st.ok() && !c.plans.pm.gather) st.hip(hipMemcpyAsync(&down->value, w.value_words, sizeof(sample::Words), hipMemcpyDeviceToHost, s));
    if (st.ok() && copy) st.hip(hipMemcpyAsync(acc, w.smp.out, copy * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st.ok() && copy && phi) st.hip(hipMemcpyAsync(phi, w.phi, copy * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st.ok() && copy && cls) st.hip(hipMemcpyAsync(cls, w.smp.cls, copy, hipMemcpyDeviceToHost, s));
}

namespace {

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
    size_t live = 0;
    const hipError_t e = live_rows(h, sh, n_upper, &live);
    HIP_TRY(h, e);
    if (const int rc = row_frame(h, "nbody_pm_field", "acc", live, acc, cap, n_out)) return rc;
    if (counts) std::fill(counts, counts + 8, uint64_t(0));
    if (!live) return NBODY_OK;
    const Call c(spec, pm, true);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, n_upper, c.g, c.shape, c.deconvolve, c.op, c.plans)));
    const Scratch w = scratch_layout(scratch.get(), n_upper, n_upper, c.g, c.shape, c.deconvolve, c.op, c.plans);
    const hipStream_t s = h->stream;
    Enqueued st;
    Tally tally;
    sample::launch_stage<F>(s, sh, int(n_upper), w.smp);
    const int* order = enqueue_shared_order(h, c, sh.own_count(), n_upper, c.plans.shared, w, st, tally);
    enqueue_grid<F>(h, sh, n_upper, spec, pm, c, w, order, st, tally);
    enqueue_rows(h, c, sh.own_count(), n_upper, phi != nullptr, c.plans.shared, w, st, tally);
    Down down;
    if (st.ok()) st.hip(hipMemcpyAsync(&down.dep, w.dep.words, sizeof(deposit::Words), hipMemcpyDeviceToHost, s));
    enqueue_down(h, st, c, w, live, acc, phi, cls, &down);
    if (const int rc = st.finish(h, "nbody_pm_field")) return rc;
    if (counts) {
        std::copy(down.dep.counts, down.dep.counts + 4, counts);
        std::copy(down.rows.counts, down.rows.counts + 4, counts + 4);
    }
    record(h, c, down.rows.reads + down.value.reads, tally.sorts);
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
    uint64_t reads = 0, counted[4] = {0, 0, 0, 0};
    Enqueued st;
    Tally tally;
    Down down;
    enqueue_grid<F>(h, sh, n_upper, spec, pm, c, w, nullptr, st, tally);
    if (st.ok()) st.hip(hipMemcpyAsync(&down.dep, w.dep.words, sizeof(deposit::Words), hipMemcpyDeviceToHost, s));
    size_t at0 = 0;
    do {   // (every pass ends in Enqueued::finish: the batch's buffers are reused by the next one)
        const size_t n = std::min(batch, n_points - at0);
        if (st.ok() && n) {
            st.hip(hipMemcpyAsync(w.smp.xyz, xyz + 3 * at0, n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
            enqueue_rows(h, c, nullptr, n, phi != nullptr, false, w, st, tally);
            enqueue_down(h, st, c, w, n, acc + 3 * at0, phi ? phi + at0 : nullptr, cls ? cls + at0 : nullptr, &down);
        }
        if (const int rc = st.finish(h, "nbody_pm_field_at")) return rc;
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
    record(h, c, reads, tally.sorts);
    return NBODY_OK;
}

template void enqueue_grid<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const Call&, const Scratch&,
                                  const int*, Enqueued&, Tally&, int);
template void enqueue_grid<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const Call&, const Scratch&,
                                   const int*, Enqueued&, Tally&, int);
template int at_bodies<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, double*, double*, uint8_t*,
                              size_t, size_t*, uint64_t*);
template int at_bodies<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, double*, double*, uint8_t*,
                               size_t, size_t*, uint64_t*);
template int at_points<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const double*, size_t, double*,
                              double*, uint8_t*, uint64_t*);
template int at_points<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyPmSpec&, const double*, size_t, double*,
                               double*, uint8_t*, uint64_t*);

}}  // namespace nbody::pm
