// nbody_poisson.cpp -- nbody_grid_poisson (include/nbody_hip.h, "grid Poisson"): the tables made on the host, the scratch of a
// call, the one copy of the grid up, the launches of kernels_poisson.hip and the one copy down.  The host twin is poisson_grid.h's.
#include "nbody_poisson.h"

#include <string>

namespace nbody { namespace poisson {

hipError_t upload_tables(NbodyHandle* h, const Tables& t, const Scratch& w) {
    const auto upload = [h](auto* dst, const auto& src) {
        return src.empty() ? hipSuccess : hipMemcpyAsync(dst, src.data(), src.size() * sizeof(src[0]), hipMemcpyHostToDevice, h->stream);
    };
    hipError_t e = hipSuccess;
    for (int c = 0; c < 3 && e == hipSuccess; ++c) {
        e = upload(w.tw[c], t.tw[c]);
        if (e == hipSuccess) e = upload(w.K[c], t.K[c]);
        if (e == hipSuccess) e = upload(w.D[c], t.D[c]);
    }
    return e;
}

hipError_t enqueue(NbodyHandle* h, const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const Shape& sh, const Tables& t, const Plan& plan,
                   const Scratch& w, int* launches_out, int* transforms_out, int held, bool split) {
    const bool deconvolve = sh.periodic && (ps.deconvolve > 0 || split);
    hipError_t e = (held & kHeldTables) ? hipSuccess : upload_tables(h, t, w);
    int launches = 0, transforms = 2;
    if (e == hipSuccess) {
        launch_load(h->stream, sh, w);
        launches += launch_transform(h->stream, sh, plan, w.x, w, false);
        if (sh.periodic) {
            launch_green(h->stream, sh, t.c, deconvolve, w);
        } else {
            if (!(held & kHeldKernel)) {
                launch_kernel(h->stream, sh, spec.spacing, ps.soften, w);
                launches += launch_transform(h->stream, sh, plan, w.k, w, false);
                transforms = 3;
            }
            launch_mul(h->stream, sh, w);
        }
        launches += launch_transform(h->stream, sh, plan, w.x, w, true);
        launch_store(h->stream, sh, ps.g, t.inv_points, w);
        e = hipGetLastError();
    }
    if (launches_out) *launches_out = launches;
    if (transforms_out) *transforms_out = transforms;
    return e;
}

int solve(NbodyHandle* h, const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const double* mass, double* phi) {
    const Shape sh = shape_of(spec);
    const Tables t = tables_of(spec, ps, sh);
    const Plan plan = make_plan();
    const bool deconvolve = sh.periodic && ps.deconvolve > 0;
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(sh, deconvolve)));
    const Scratch w = scratch_layout(scratch.get(), sh, deconvolve);
    // the grid on its way to the device (t outlives the call's synchronisation)
    Enqueued st;
    st.hip(hipMemcpyAsync(w.real, mass, sh.cells() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int launches = 0, transforms = 2;
    if (st.ok()) st.hip(enqueue(h, spec, ps, sh, t, plan, w, &launches, &transforms));
    if (st.ok()) st.hip(hipMemcpyAsync(phi, w.real, sh.cells() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (const int rc = st.finish(h, "nbody_grid_poisson")) return rc;
    h->poisson_last[0] = 1;
    h->poisson_last[1] = uint64_t(plan.code());
    h->poisson_last[2] = uint64_t(launches);
    h->poisson_last[3] = uint64_t(sh.points()) * uint64_t(transforms);
    return NBODY_OK;
}

}}  // namespace nbody::poisson
