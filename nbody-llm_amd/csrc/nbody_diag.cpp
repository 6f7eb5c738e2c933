// nbody_diag.cpp -- nbody_moments and nbody_lagrangian_radii (include/nbody_hip.h, "diagnostics of the state as a whole"): the
// scratch of a call, the launches of kernels_diag.hip and the host's share of the sums (the blocks in ascending order).
#include "nbody_diag.h"

#include <cmath>
#include <limits>
#include <vector>

namespace nbody { namespace diag {

const char* refusal(const NbodyHandle* h) {
    if (h->let || h->cfg.shard_mode != NBODY_SHARD_INDEX) return "NBODY_SHARD_SPATIAL handles are not accepted (out of scope)";
    if (h->cfg.world_size != 1) return "handles of a multi-rank world are not accepted (out of scope)";
    return nullptr;
}

template <class F>
int moments(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double out[10]) {
    for (int q = 0; q < kMoments; ++q) out[q] = 0.0;
    const size_t blocks = size_t(blocks_for(int(n_upper)));
    if (!blocks) return NBODY_OK;
    ScratchDev scratch(h->mem);   // [blocks][kMoments] block sums
    HIP_TRY(h, scratch.alloc(blocks * kMoments * sizeof(double)));
    double* d = scratch.get<double>();
    launch_diag_moments<F>(h->stream, sh, int(n_upper), d);
    std::vector<double> part(blocks * kMoments);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(part.data(), d, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < blocks; ++b)   // blocks in ascending order
        for (int q = 0; q < kMoments; ++q) out[q] += part[b * kMoments + q];
    return NBODY_OK;
}
template int moments<float>(NbodyHandle*, const ShardT<float>&, size_t, double*);
template int moments<double>(NbodyHandle*, const ShardT<double>&, size_t, double*);

template <class F>
int lagrangian_radii(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const double* center, const double* fractions, size_t n_frac,
                     double* radii, double* mass_out) {
    if (mass_out) *mass_out = 0.0;
    for (size_t k = 0; k < n_frac; ++k) radii[k] = std::numeric_limits<double>::quiet_NaN();
    if (!n_upper) return NBODY_OK;   // no body in the order
    double c[3];
    if (center) { c[0] = center[0]; c[1] = center[1]; c[2] = center[2]; }
    else {
        double mom[kMoments];
        int rc = moments<F>(h, sh, n_upper, mom);
        if (rc) return rc;
        for (int k = 0; k < 3; ++k) c[k] = mom[1 + k] / mom[0];
    }
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(radii_scratch_bytes(n_upper, n_frac)));
    const RadiiScratch w = radii_scratch_layout(scratch.get(), n_upper, n_frac);
    std::vector<double> out(n_frac + 1);
    // (c, fractions and out are pageable: the copies return once the data has left or reached them)
    hipError_t e = hipMemcpyAsync(w.center, c, sizeof(c), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && n_frac) e = hipMemcpyAsync(w.fractions, fractions, n_frac * sizeof(double), hipMemcpyHostToDevice, h->stream);
    bool sort_failed = false;
    if (e == hipSuccess) {
        sort_failed = launch_diag_radii<F>(h->stream, sh, int(n_upper), int(n_frac), w) != 0;
        e = hipGetLastError();
    }
    if (e == hipSuccess && !sort_failed) e = hipMemcpyAsync(out.data(), w.out, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_sync = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = e_sync;
    HIP_TRY(h, e);
    if (sort_failed) return fail(h, NBODY_ERR_HIP, "nbody_lagrangian_radii: rocPRIM call failed");
    for (size_t k = 0; k < n_frac; ++k) radii[k] = out[k];
    if (mass_out) *mass_out = out[n_frac];
    return NBODY_OK;
}
template int lagrangian_radii<float>(NbodyHandle*, const ShardT<float>&, size_t, const double*, const double*, size_t, double*, double*);
template int lagrangian_radii<double>(NbodyHandle*, const ShardT<double>&, size_t, const double*, const double*, size_t, double*, double*);

}}  // namespace nbody::diag
