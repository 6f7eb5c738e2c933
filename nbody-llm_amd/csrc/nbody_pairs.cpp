// nbody_pairs.cpp -- nbody_partners and nbody_bound_pairs (include/nbody_hip.h, "binary census"): the scratch of a call, the
// launches of kernels_pairs.hip, and the copies of what the caller asked for -- n partners, or the n_pairs records of the list.
#include "nbody_pairs.h"

#include <algorithm>
#include <vector>

namespace nbody { namespace pairs {

namespace {
// the live count of sh, at most n_upper (a copy of the device's word; the host's view of the count is left as it is)
template <class F>
hipError_t read_live(NbodyHandle* h, const ShardT<F>& sh, int* live) {
    hipError_t e = hipMemcpyAsync(live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    return e;
}
}  // namespace

template <class F>
int partners(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, int32_t* partner, double* energy, size_t cap,
             size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!n_upper) return NBODY_OK;
    int live = 0;
    if (!partner && !energy) {   // counts only
        HIP_TRY(h, read_live(h, sh, &live));
        if (n_out) *n_out = std::min(size_t(std::max(live, 0)), n_upper);
        return NBODY_OK;
    }
    const PartnerPlan plan = make_partner_plan(int(n_upper));
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, plan, false)));
    const PairScratch w = scratch_layout(scratch.get(), n_upper, plan, false);
    launch_partners<F>(h->stream, sh, int(n_upper), plan, g, g_soft * g_soft, w);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, read_live(h, sh, &live));
    const size_t n = std::min(size_t(std::max(live, 0)), n_upper);
    const bool fits = n <= cap;
    // (partner and energy are pageable: the copies return once the data has reached them)
    if (fits && n && partner) HIP_TRY(h, hipMemcpyAsync(partner, w.partner, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (fits && n && energy) HIP_TRY(h, hipMemcpyAsync(energy, w.energy, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (n_out) *n_out = n;
    if (!fits) return fail(h, NBODY_ERR_CAPACITY, "nbody_partners: buffer too small");
    return NBODY_OK;
}
template int partners<float>(NbodyHandle*, const ShardT<float>&, size_t, double, double, int32_t*, double*, size_t, size_t*);
template int partners<double>(NbodyHandle*, const ShardT<double>&, size_t, double, double, int32_t*, double*, size_t, size_t*);

template <class F>
int bound_pairs(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, NbodyBoundPair* pairs, size_t cap,
                size_t* n_pairs, double* binding_sum) {
    if (n_pairs) *n_pairs = 0;
    if (binding_sum) *binding_sum = 0.0;
    if (!n_upper) return NBODY_OK;
    const PartnerPlan plan = make_partner_plan(int(n_upper));
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, plan, true)));
    const PairScratch w = scratch_layout(scratch.get(), n_upper, plan, true);
    launch_partners<F>(h->stream, sh, int(n_upper), plan, g, g_soft * g_soft, w);
    const bool scan_failed = launch_bound_pairs<F>(h->stream, sh, int(n_upper), g, w) != 0;
    int total = 0;
    HIP_TRY(h, hipGetLastError());
    if (!scan_failed) HIP_TRY(h, hipMemcpyAsync(&total, w.total, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (scan_failed) return fail(h, NBODY_ERR_HIP, "nbody_bound_pairs: rocPRIM call failed");
    const size_t np = std::min(size_t(std::max(total, 0)), n_upper / 2);
    const bool fits = !pairs || np <= cap;
    // only the np records of the list cross to the host: into the caller's buffer, or into one of the call's own when the
    // caller wants their binding energies alone
    std::vector<NbodyBoundPair> own;
    const NbodyBoundPair* list = pairs;
    if (fits && np && (pairs || binding_sum)) {
        if (!pairs) { own.resize(np); list = own.data(); }
        HIP_TRY(h, hipMemcpyAsync(const_cast<NbodyBoundPair*>(list), w.pairs, np * sizeof(NbodyBoundPair), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (n_pairs) *n_pairs = np;
    if (!fits) return fail(h, NBODY_ERR_CAPACITY, "nbody_bound_pairs: buffer too small");
    if (binding_sum) {
        double sum = 0.0;
        for (size_t k = 0; k < np; ++k) sum += list[k].binding;   // in list order
        *binding_sum = sum;
    }
    return NBODY_OK;
}
template int bound_pairs<float>(NbodyHandle*, const ShardT<float>&, size_t, double, double, NbodyBoundPair*, size_t, size_t*, double*);
template int bound_pairs<double>(NbodyHandle*, const ShardT<double>&, size_t, double, double, NbodyBoundPair*, size_t, size_t*, double*);

}}  // namespace nbody::pairs
