// nbody_p3m.cpp -- nbody_p3m_field and nbody_p3m_field_at (include/nbody_hip.h, "P3M field"): the one scratch of a call, the mesh
// stages of nbody_pm.cpp with the Gaussian split in the Poisson tables, the chain order and the pair sum of kernels_p3m.hip, the
// addition of the two parts, the copies down and the one synchronisation.  The host twin is p3m_pairs.h's.
#include "nbody_p3m.h"

#include "nbody_pm.h"
#include "nbody_sample.h"   // kPointBatch

#include <algorithm>
#include <vector>

namespace nbody { namespace p3m {

namespace {

// what a call holds on the host until its last synchronisation
struct Call {
    pm::Call mesh;
    Chain ch;
    Params params;
    Plan plan;
    std::vector<Entry> table;
    bool with_short;
    Call(const NbodyGridSpec& spec, const NbodyP3mSpec& p, bool bodies)
        : mesh(spec, p.pm, bodies, p.r_split), ch(chain_of(mesh.g, p.r_cut)), params(params_of(mesh.g, p.r_cut, p.soften)), plan(make_plan()),
          table(size_t(kIntervals) + 1), with_short(p.terms != NBODY_P3M_MESH_ONLY) {
        p3m::table(p.r_split, p.r_cut, table.data());
    }
};

// the two scratches, one after the other in one allocation
struct Both {
    pm::Scratch mesh;
    Scratch pairs;
};
size_t mesh_bytes(const Call& c, size_t n_bodies, size_t n_rows) {
    return pm::scratch_bytes(n_bodies, n_rows, c.mesh.g, c.mesh.shape, c.mesh.deconvolve, c.mesh.op, c.mesh.plans);
}
Both layout(const Call& c, void* base, size_t n_bodies, size_t n_rows, bool at_points) {
    Both w;
    w.mesh = pm::scratch_layout(base, n_bodies, n_rows, c.mesh.g, c.mesh.shape, c.mesh.deconvolve, c.mesh.op, c.mesh.plans);
    w.pairs = scratch_layout(static_cast<char*>(base) + mesh_bytes(c, n_bodies, n_rows), n_bodies, n_rows, c.ch.cells(), at_points);
    return w;
}

// the table on its way up, the words zeroed and the bodies in chain order
template <class F>
void enqueue_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const Call& c, const Both& w, Enqueued& st) {
    if (!st.ok() || !c.with_short) return;
    st.hip(hipMemcpyAsync(w.pairs.table, c.table.data(), c.table.size() * sizeof(Entry), hipMemcpyHostToDevice, h->stream));
    if (st.ok()) st.hip(hipMemsetAsync(w.pairs.words, 0, sizeof(Words), h->stream));
    if (st.ok()) st.prim(launch_body_order<F>(h->stream, sh, int(n_upper), c.mesh.g, c.ch, w.pairs));
    st.last();
}

// the pair sum at the n targets and the addition to the mesh rows of w.mesh
void enqueue_short(NbodyHandle* h, const NbodyP3mSpec& p, const Call& c, const Both& w, size_t n_bodies, size_t n, bool at_points, const int* count,
                   bool with_phi, Enqueued& st) {
    if (!st.ok() || !c.with_short || !n) return;
    launch_short(h->stream, int(n_bodies), int(n), at_points, c.plan, c.ch, c.params, p.pm.poisson.g, w.pairs);
    launch_add(h->stream, count, int(n), p.terms, w.pairs, w.mesh.smp.out, with_phi ? w.mesh.phi : nullptr);
    st.last();
}

void record(NbodyHandle* h, const Call& c, const Words& words) {
    h->p3m_last[0] = 1;
    h->p3m_last[1] = uint64_t(c.plan.lds) | uint64_t(c.mesh.plans.pm.gather | (c.mesh.plans.shared ? 2 : 0)) << 1;
    h->p3m_last[2] = words.looked;
    h->p3m_last[3] = words.counted;
}

}  // namespace

template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyP3mSpec& p3m, double* acc, double* phi,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts) {
    // the live count first: a call that is refused, a buffer that is too small included, computes and writes nothing
    size_t live = 0;
    const hipError_t e = live_rows(h, sh, n_upper, &live);
    HIP_TRY(h, e);
    if (const int rc = row_frame(h, "nbody_p3m_field", "acc", live, acc, cap, n_out)) return rc;
    if (counts) std::fill(counts, counts + 8, uint64_t(0));
    if (!live) return NBODY_OK;
    const Call c(spec, p3m, true);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(mesh_bytes(c, n_upper, n_upper) + scratch_bytes(n_upper, n_upper, c.ch.cells(), false)));
    const Both w = layout(c, scratch.get(), n_upper, n_upper, false);
    const hipStream_t s = h->stream;
    Enqueued st;
    pm::Tally tally;
    // the mesh part: nbody_pm_field's stages, the split in the tables
    sample::launch_stage<F>(s, sh, int(n_upper), w.mesh.smp);
    const int* order = pm::enqueue_shared_order(h, c.mesh, sh.own_count(), n_upper, c.mesh.plans.shared, w.mesh, st, tally);
    pm::enqueue_grid<F>(h, sh, n_upper, spec, p3m.pm, c.mesh, w.mesh, order, st, tally);
    pm::enqueue_rows(h, c.mesh, sh.own_count(), n_upper, phi != nullptr, c.mesh.plans.shared, w.mesh, st, tally);
    // the short-range part, added to the rows
    enqueue_bodies<F>(h, sh, n_upper, c, w, st);
    enqueue_short(h, p3m, c, w, n_upper, n_upper, false, sh.own_count(), phi != nullptr, st);
    pm::Down down;
    Words words{};
    if (st.ok()) st.hip(hipMemcpyAsync(&down.dep, w.mesh.dep.words, sizeof(deposit::Words), hipMemcpyDeviceToHost, s));
    if (st.ok() && c.with_short) st.hip(hipMemcpyAsync(&words, w.pairs.words, sizeof(Words), hipMemcpyDeviceToHost, s));
    pm::enqueue_down(h, st, c.mesh, w.mesh, live, acc, phi, cls, &down);
    if (const int rc = st.finish(h, "nbody_p3m_field")) return rc;
    if (counts) {
        std::copy(down.dep.counts, down.dep.counts + 4, counts);
        std::copy(down.rows.counts, down.rows.counts + 4, counts + 4);
    }
    record(h, c, words);
    return NBODY_OK;
}

template <class F>
int at_points(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyP3mSpec& p3m, const double* xyz,
              size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts) {
    if (counts) std::fill(counts, counts + 8, uint64_t(0));
    const Call c(spec, p3m, false);
    const size_t batch = std::max<size_t>(std::min(n_points, sample::kPointBatch), 1);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(mesh_bytes(c, n_upper, batch) + scratch_bytes(n_upper, batch, c.ch.cells(), true)));
    const Both w = layout(c, scratch.get(), n_upper, batch, true);
    const hipStream_t s = h->stream;
    uint64_t counted[4] = {0, 0, 0, 0};
    Enqueued st;
    pm::Tally tally;
    pm::Down down;
    Words words{};
    pm::enqueue_grid<F>(h, sh, n_upper, spec, p3m.pm, c.mesh, w.mesh, nullptr, st, tally);
    if (st.ok()) st.hip(hipMemcpyAsync(&down.dep, w.mesh.dep.words, sizeof(deposit::Words), hipMemcpyDeviceToHost, s));
    enqueue_bodies<F>(h, sh, n_upper, c, w, st);
    size_t at0 = 0;
    do {   // (every pass ends in Enqueued::finish: the batch's buffers are reused by the next one)
        const size_t n = std::min(batch, n_points - at0);
        if (st.ok() && n) {
            st.hip(hipMemcpyAsync(w.mesh.smp.xyz, xyz + 3 * at0, n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
            pm::enqueue_rows(h, c.mesh, nullptr, n, phi != nullptr, false, w.mesh, st, tally);
            if (st.ok() && c.with_short) {
                st.prim(launch_point_order(s, w.mesh.smp.xyz, int(n), c.mesh.g, c.ch, w.pairs));
                st.last();
            }
            enqueue_short(h, p3m, c, w, n_upper, n, true, nullptr, phi != nullptr, st);
            if (st.ok() && c.with_short) st.hip(hipMemcpyAsync(&words, w.pairs.words, sizeof(Words), hipMemcpyDeviceToHost, s));   // (it runs on)
            pm::enqueue_down(h, st, c.mesh, w.mesh, n, acc + 3 * at0, phi ? phi + at0 : nullptr, cls ? cls + at0 : nullptr, &down);
        }
        if (const int rc = st.finish(h, "nbody_p3m_field_at")) return rc;
        for (int k = 0; k < 4; ++k) counted[k] += down.rows.counts[k];
        down.rows = sample::Words{};
        down.value = sample::Words{};
        at0 += n;
    } while (at0 < n_points);
    if (counts) {
        std::copy(down.dep.counts, down.dep.counts + 4, counts);
        std::copy(counted, counted + 4, counts + 4);
    }
    record(h, c, words);
    return NBODY_OK;
}

template int at_bodies<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyP3mSpec&, double*, double*, uint8_t*,
                              size_t, size_t*, uint64_t*);
template int at_bodies<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyP3mSpec&, double*, double*, uint8_t*,
                               size_t, size_t*, uint64_t*);
template int at_points<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const NbodyP3mSpec&, const double*, size_t, double*,
                              double*, uint8_t*, uint64_t*);
template int at_points<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const NbodyP3mSpec&, const double*, size_t, double*,
                               double*, uint8_t*, uint64_t*);

}}  // namespace nbody::p3m
