// nbody_pairs.cpp -- nbody_partners and nbody_bound_pairs (include/nbody_hip.h, "binary census"): the scratch of a call, the
// launches of kernels_pairs.hip, and the copies of what the caller asked for -- n partners, or the n_pairs records of the list.
// nbody_nearest, nbody_contacts and nbody_merge_contacts ("sticky mergers") are the same three steps under the distance metric,
// and the last one then writes the merged records and runs the handle's retain.
#include "nbody_pairs.h"
#include "nbody_cells.h"

#include <algorithm>
#include <string>
#include <vector>

namespace nbody { namespace pairs {

template <class F>
int partners(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, int32_t* partner, double* energy, size_t cap,
             size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!n_upper) return NBODY_OK;
    size_t n = 0;
    if (!partner && !energy) {   // counts only
        HIP_TRY(h, live_rows(h, sh, n_upper, &n));
        if (n_out) *n_out = n;
        return NBODY_OK;
    }
    const PartnerPlan plan = make_partner_plan(int(n_upper));
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, plan, false)));
    const PairScratch w = scratch_layout(scratch.get(), n_upper, plan, false);
    launch_partners<F>(h->stream, sh, int(n_upper), plan, g, g_soft * g_soft, w);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, live_rows(h, sh, n_upper, &n));
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

// ---- sticky mergers
template <class F>
int nearest(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int32_t* nearest_out, double* dist2, size_t cap, size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!n_upper) return NBODY_OK;
    size_t n = 0;
    if (!nearest_out && !dist2) {   // counts only
        HIP_TRY(h, live_rows(h, sh, n_upper, &n));
        if (n_out) *n_out = n;
        return NBODY_OK;
    }
    const PartnerPlan plan = make_partner_plan(int(n_upper));
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, plan, false)));
    const PairScratch w = scratch_layout(scratch.get(), n_upper, plan, false);
    launch_nearest<F>(h->stream, sh, int(n_upper), plan, w);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, live_rows(h, sh, n_upper, &n));
    const bool fits = n <= cap;
    if (fits && n && nearest_out) HIP_TRY(h, hipMemcpyAsync(nearest_out, w.partner, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (fits && n && dist2) HIP_TRY(h, hipMemcpyAsync(dist2, w.energy, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (n_out) *n_out = n;
    if (!fits) return fail(h, NBODY_ERR_CAPACITY, "nbody_nearest: buffer too small");
    return NBODY_OK;
}
template int nearest<float>(NbodyHandle*, const ShardT<float>&, size_t, int32_t*, double*, size_t, size_t*);
template int nearest<double>(NbodyHandle*, const ShardT<double>&, size_t, int32_t*, double*, size_t, size_t*);

namespace {
// the scratch of a call, the nearest pass and the contact list on the device: *np contacts among *live bodies (n_upper > 0)
template <class F>
int find_contacts(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, const char* call, ScratchDev& scratch, PairScratch* w,
                  size_t* np, size_t* live_out) {
    const PartnerPlan plan = make_partner_plan(int(n_upper));
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, plan, true)));
    *w = scratch_layout(scratch.get(), n_upper, plan, true);
    // every body's nearest: within the radius over the cells of a grid when the handle asks for it and one can be drawn
    // (nbody_cells.h: a contact is a mutual nearest pair inside the radius either way), else over all pairs
    cells::Search search(h->mem);
    cells::Counters counted;
    int rc = cells::prepare<F>(h, sh, n_upper, radius, call, &search);
    if (rc) return rc;
    if (search.on) cells::launch_nearest_within(h->stream, int(n_upper), search.n_gridded, radius * radius, search.w, *w);
    else launch_nearest<F>(h->stream, sh, int(n_upper), plan, *w);
    const bool scan_failed = launch_contacts<F>(h->stream, sh, int(n_upper), radius * radius, *w) != 0;
    int total = 0, live = 0;
    HIP_TRY(h, hipGetLastError());
    if (!scan_failed) HIP_TRY(h, hipMemcpyAsync(&total, w->total, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    rc = cells::fetch_counters(h, search, &counted);   // and the synchronisation
    if (rc) return rc;
    if (scan_failed) return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
    cells::record(h, search, counted);
    *live_out = std::min(size_t(std::max(live, 0)), n_upper);
    *np = std::min(size_t(std::max(total, 0)), *live_out / 2);
    return NBODY_OK;
}

// the np records of the list to the caller, `into` filled: i minus the absorbed bodies below i
int copy_contacts(NbodyHandle* h, const PairScratch& w, NbodyContact* list, size_t np) {
    if (!list || !np) return NBODY_OK;
    HIP_TRY(h, hipMemcpyAsync(list, w.contacts, np * sizeof(NbodyContact), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> gone(np);
    for (size_t k = 0; k < np; ++k) gone[k] = list[k].j;
    std::sort(gone.begin(), gone.end());
    for (size_t k = 0; k < np; ++k) list[k].into = list[k].i - int32_t(std::lower_bound(gone.begin(), gone.end(), list[k].i) - gone.begin());
    return NBODY_OK;
}
}  // namespace

template <class F>
int contacts(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, NbodyContact* list, size_t cap, size_t* n_contacts) {
    if (n_contacts) *n_contacts = 0;
    if (!n_upper) return NBODY_OK;
    ScratchDev scratch(h->mem);
    PairScratch w;
    size_t np = 0, live = 0;
    int rc = find_contacts<F>(h, sh, n_upper, radius, "nbody_contacts", scratch, &w, &np, &live);
    if (rc) return rc;
    if (n_contacts) *n_contacts = np;
    if (list && np > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_contacts: buffer too small");
    return copy_contacts(h, w, list, np);
}
template int contacts<float>(NbodyHandle*, const ShardT<float>&, size_t, double, NbodyContact*, size_t, size_t*);
template int contacts<double>(NbodyHandle*, const ShardT<double>&, size_t, double, NbodyContact*, size_t, size_t*);

template <class F>
int merge_contacts(NbodyHandle* h, BodyStore<F>& b, double radius, NbodyContact* list, size_t cap, size_t* n_contacts,
                   typename ShardT<F>::V4* jerk, void (*retain)(NbodyHandle*, int)) {
    if (n_contacts) *n_contacts = 0;
    const size_t n_upper = b.n_local;
    if (!n_upper) return NBODY_OK;
    ScratchDev scratch(h->mem);
    PairScratch w;
    size_t np = 0, live = 0;
    int rc = find_contacts<F>(h, b.sh, n_upper, radius, "nbody_merge_contacts", scratch, &w, &np, &live);
    if (rc) return rc;
    if (n_contacts) *n_contacts = np;
    if (list && np > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_merge_contacts: buffer too small");
    if (!np) return NBODY_OK;   // (nothing of the handle's has been written, its view of the count included)
    launch_merge<F>(h->stream, b.sh, jerk, int(n_upper), w);
    retain(h, int(n_upper));
    HIP_TRY(h, hipGetLastError());
    rc = copy_contacts(h, w, list, np);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    b.set_own_count(live - np);   // exact: the retain dropped the np absorbed bodies of `live`
    return NBODY_OK;
}
template int merge_contacts<float>(NbodyHandle*, BodyStore<float>&, double, NbodyContact*, size_t, size_t*, float4*, void (*)(NbodyHandle*, int));
template int merge_contacts<double>(NbodyHandle*, BodyStore<double>&, double, NbodyContact*, size_t, size_t*, double4*, void (*)(NbodyHandle*, int));

}}  // namespace nbody::pairs
