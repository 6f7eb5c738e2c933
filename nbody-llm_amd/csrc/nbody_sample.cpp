// nbody_sample.cpp -- nbody_grid_sample and nbody_grid_sample_at (include/nbody_hip.h, "grid sample"): the scratch of a call,
// the copy of the grid to the device, the launches of kernels_sample.hip and the copies back.  The host twin is sample_grid.h's.
#include "nbody_sample.h"

#include <algorithm>
#include <string>

namespace nbody { namespace sample {

namespace {

// The grid on its way to the device and, under sample_pregrad, the difference grids after it.
hipError_t upload_grid(NbodyHandle* h, const Grid& g, const double* grid, int fields, int op, const Plan& plan, const Scratch& w) {
    const hipError_t e = hipMemcpyAsync(w.grid, grid, size_t(fields) * cells_of(g) * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return e;
    if (plan.pregrad) launch_diff(h->stream, g, op, w);
    return hipGetLastError();
}

// The passes over the n rows of w.xyz (count: the live rows' word on the device, or null: all n), the copy of the first `copy`
// rows to out and cls and of the words, and the synchronisation (Enqueued::finish).
int passes(NbodyHandle* h, const char* call, const Grid& g, int fields, int op, const Plan& plan, const Scratch& w, const int* count, size_t n,
           size_t copy, double* out, uint8_t* cls, Words* words) {
    Enqueued st;
    st.prim(launch_sample(h->stream, count, int(n), g, fields, op, plan, w));
    const size_t width = size_t(width_of(op, fields));
    st.last();
    if (st.ok()) st.hip(hipMemcpyAsync(words, w.words, sizeof(Words), hipMemcpyDeviceToHost, h->stream));
    if (st.ok() && copy) st.hip(hipMemcpyAsync(out, w.out, copy * width * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (st.ok() && copy && cls) st.hip(hipMemcpyAsync(cls, w.cls, copy, hipMemcpyDeviceToHost, h->stream));
    return st.finish(h, call);
}

void record(NbodyHandle* h, const Plan& plan, uint64_t reads) {
    h->sample_last[0] = 1;
    h->sample_last[1] = uint64_t(plan.code());
    h->sample_last[2] = reads;
    h->sample_last[3] = 0;
}

}  // namespace

template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const double* grid, int fields, int op, double* out,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts) {
    // the live count first: a call that is refused, a buffer that is too small included, computes and writes nothing
    size_t live = 0;
    const hipError_t e = live_rows(h, sh, n_upper, &live);
    HIP_TRY(h, e);
    if (const int rc = row_frame(h, "nbody_grid_sample", "out", live, out, cap, n_out)) return rc;
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!live) return NBODY_OK;
    const Grid g = deposit::grid_of(spec);
    const size_t cells = cells_of(g);
    const Plan plan = make_plan(op, cells);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, cells, fields, op, plan)));
    const Scratch w = scratch_layout(scratch.get(), n_upper, cells, fields, op, plan);
    HIP_TRY(h, upload_grid(h, g, grid, fields, op, plan, w));
    launch_stage<F>(h->stream, sh, int(n_upper), w);
    Words words{};
    const int rc = passes(h, "nbody_grid_sample", g, fields, op, plan, w, sh.own_count(), n_upper, live, out, cls, &words);
    if (rc) return rc;
    if (counts) std::copy(words.counts, words.counts + 4, counts);
    record(h, plan, words.reads);
    return NBODY_OK;
}
template int at_bodies<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, const double*, int, int, double*, uint8_t*, size_t,
                              size_t*, uint64_t*);
template int at_bodies<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, const double*, int, int, double*, uint8_t*, size_t,
                               size_t*, uint64_t*);

int at_points(NbodyHandle* h, const NbodyGridSpec& spec, const double* grid, int fields, int op, const double* xyz, size_t n_points, double* out,
              uint8_t* cls, uint64_t* counts) {
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!n_points) return NBODY_OK;
    const Grid g = deposit::grid_of(spec);
    const size_t cells = cells_of(g), width = size_t(width_of(op, fields));
    const Plan plan = make_plan(op, cells);
    const size_t batch = std::min(n_points, kPointBatch);
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(batch, cells, fields, op, plan)));
    const Scratch w = scratch_layout(scratch.get(), batch, cells, fields, op, plan);
    HIP_TRY(h, upload_grid(h, g, grid, fields, op, plan, w));
    uint64_t counted[4] = {0, 0, 0, 0}, reads = 0;
    for (size_t at0 = 0; at0 < n_points; at0 += batch) {
        const size_t n = std::min(batch, n_points - at0);
        HIP_TRY(h, hipMemcpyAsync(w.xyz, xyz + 3 * at0, n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        Words words{};
        const int rc = passes(h, "nbody_grid_sample_at", g, fields, op, plan, w, nullptr, n, n, out + at0 * width, cls ? cls + at0 : nullptr, &words);
        if (rc) return rc;   // (synchronised: the batch's buffers are reused by the next one)
        for (int k = 0; k < 4; ++k) counted[k] += words.counts[k];
        reads += words.reads;
    }
    if (counts) std::copy(counted, counted + 4, counts);
    record(h, plan, reads);
    return NBODY_OK;
}

}}  // namespace nbody::sample
