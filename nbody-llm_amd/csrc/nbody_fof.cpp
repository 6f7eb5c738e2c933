// nbody_fof.cpp -- nbody_fof_labels and nbody_fof_groups (include/nbody_hip.h, "friends-of-friends groups"): the scratch of a
// call, the launches of kernels_fof.hip, and the copies of what the caller asked for -- n labels, or the listed records and
// their members; and nbody_fof_bound_groups ("self-bound subsets of friends-of-friends groups"): the same catalogue, then the
// pass loop of kernels_unbind.hip.
#include "nbody_fof.h"
#include "kernels_unbind.h"
#include "nbody_cells.h"

#include <algorithm>
#include <string>

namespace nbody { namespace fof {

namespace {
// the components and the catalogue of sh's bodies on the device, and what the host needs to size the read-back: the live
// count and {listed groups, their members} (n_upper > 0)
template <class F>
int find_groups(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double linking_length, int min_members, bool sort, const char* call,
                ScratchDev& scratch, FofScratch* w, size_t* live_out, size_t* n_groups, size_t* n_members) {
    const pairs::PartnerPlan plan = pairs::make_partner_plan(int(n_upper));
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper)));
    *w = scratch_layout(scratch.get(), n_upper);
    // the links: over the cells of a grid when the handle asks for it and one can be drawn (nbody_cells.h), else over all pairs
    cells::Search search(h->mem);
    cells::Counters counted;
    int rc = cells::prepare<F>(h, sh, n_upper, linking_length, call, &search);
    if (rc) return rc;
    if (search.on) cells::launch_link_components(h->stream, sh.own_count(), int(n_upper), search.n_gridded, linking_length * linking_length, search.w, *w);
    else launch_components<F>(h->stream, sh, int(n_upper), plan, linking_length * linking_length, *w);
    const bool prim_failed = launch_catalogue(h->stream, int(n_upper), min_members, sort, *w) != 0;
    int total[2] = {0, 0}, live = 0;
    HIP_TRY(h, hipGetLastError());
    if (!prim_failed) HIP_TRY(h, hipMemcpyAsync(total, w->total, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    rc = cells::fetch_counters(h, search, &counted);   // and the synchronisation
    if (rc) return rc;
    if (prim_failed) return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
    cells::record(h, search, counted);
    *live_out = std::min(size_t(std::max(live, 0)), n_upper);
    *n_members = std::min(size_t(std::max(total[1], 0)), *live_out);
    *n_groups = std::min(size_t(std::max(total[0], 0)), *n_members);
    return NBODY_OK;
}
}  // namespace

template <class F>
int labels(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double linking_length, int32_t* label, size_t cap, size_t* n_out,
           size_t* n_groups_out) {
    if (n_out) *n_out = 0;
    if (n_groups_out) *n_groups_out = 0;
    if (!n_upper) return NBODY_OK;
    if (!label && !n_groups_out) {   // the bodies only
        int live = 0;
        HIP_TRY(h, hipMemcpyAsync(&live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (n_out) *n_out = std::min(size_t(std::max(live, 0)), n_upper);
        return NBODY_OK;
    }
    ScratchDev scratch(h->mem);
    FofScratch w;
    size_t n = 0, n_groups = 0, n_members = 0;
    // (every component is listed with min_members = 1: the listed groups are the components)
    int rc = find_groups<F>(h, sh, n_upper, linking_length, 1, false, "nbody_fof_labels", scratch, &w, &n, &n_groups, &n_members);
    if (rc) return rc;
    if (n_out) *n_out = n;
    if (n_groups_out) *n_groups_out = n_groups;
    if (label && n > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_fof_labels: buffer too small");
    if (label && n) {   // (label is pageable: the copy returns once the data has reached it)
        HIP_TRY(h, hipMemcpyAsync(label, w.label, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return NBODY_OK;
}
template int labels<float>(NbodyHandle*, const ShardT<float>&, size_t, double, int32_t*, size_t, size_t*, size_t*);
template int labels<double>(NbodyHandle*, const ShardT<double>&, size_t, double, int32_t*, size_t, size_t*, size_t*);

template <class F>
int groups(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double linking_length, int min_members, NbodyGroup* list,
           size_t group_cap, size_t* n_groups_out, int32_t* members, size_t member_cap, size_t* n_members_out) {
    if (n_groups_out) *n_groups_out = 0;
    if (n_members_out) *n_members_out = 0;
    if (!n_upper) return NBODY_OK;
    ScratchDev scratch(h->mem), records(h->mem);
    FofScratch w;
    size_t n = 0, n_groups = 0, n_members = 0;
    int rc = find_groups<F>(h, sh, n_upper, linking_length, min_members, list || members, "nbody_fof_groups", scratch, &w, &n, &n_groups,
                            &n_members);
    if (rc) return rc;
    if (n_groups_out) *n_groups_out = n_groups;
    if (n_members_out) *n_members_out = n_members;
    if ((list && n_groups > group_cap) || (members && n_members > member_cap))
        return fail(h, NBODY_ERR_CAPACITY, "nbody_fof_groups: buffer too small");
    // only the listed records and members cross to the host
    if (list && n_groups) {
        HIP_TRY(h, records.alloc(n_groups * sizeof(NbodyGroup)));
        launch_sums<F>(h->stream, sh, int(n_upper), int(n_groups), w, records.get<NbodyGroup>());
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(list, records.get<NbodyGroup>(), n_groups * sizeof(NbodyGroup), hipMemcpyDeviceToHost, h->stream));
    }
    if (members && n_members)
        HIP_TRY(h, hipMemcpyAsync(members, w.members(n_upper), n_members * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}
template int groups<float>(NbodyHandle*, const ShardT<float>&, size_t, double, int, NbodyGroup*, size_t, size_t*, int32_t*, size_t, size_t*);
template int groups<double>(NbodyHandle*, const ShardT<double>&, size_t, double, int, NbodyGroup*, size_t, size_t*, int32_t*, size_t, size_t*);

template <class F>
int bound_groups(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, double g_soft, double linking_length, int min_members,
                 int max_iterations, NbodyBoundGroup* list, size_t group_cap, size_t* n_groups_out, int32_t* members, size_t member_cap,
                 size_t* n_members_out, double* energy) {
    static const char* const call = "nbody_fof_bound_groups";
    if (n_groups_out) *n_groups_out = 0;
    if (n_members_out) *n_members_out = 0;
    if (!n_upper) return NBODY_OK;
    ScratchDev scratch(h->mem), passes(h->mem);
    FofScratch w;
    size_t n = 0, fof_groups = 0, fof_members = 0;
    // step 0: the catalogue and the member list of nbody_fof_groups, on the device
    int rc = find_groups<F>(h, sh, n_upper, linking_length, min_members, true, call, scratch, &w, &n, &fof_groups, &fof_members);
    if (rc) return rc;
    if (!fof_groups) return NBODY_OK;
    const int n_members = int(fof_members), n_groups = int(fof_groups);
    HIP_TRY(h, passes.alloc(unbind_scratch_bytes(fof_members, fof_groups)));
    const UnbindScratch u = unbind_layout(passes.get(), fof_members, fof_groups);
    launch_unbind_init(h->stream, n_members, n_groups, w, u);
    // the passes: one launch chain serves every group still running; the host reads back how many go on
    for (int pass = 0; pass < max_iterations; ++pass) {
        int running = 0;
        HIP_TRY(h, hipMemsetAsync(u.counters, 0, sizeof(int), h->stream));
        launch_unbind_pass<F>(h->stream, sh, int(n_upper), n_members, n_groups, min_members, pass, pass + 1 == max_iterations, g,
                              g_soft * g_soft, w, u);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(&running, u.counters, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (running <= 0) break;
    }
    if (launch_unbind_finish(h->stream, int(n_upper), n_members, n_groups, min_members, w, u) != 0)
        return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
    int total[2] = {0, 0};
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(total, u.counters + 1, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t bound_members = std::min(size_t(std::max(total[1], 0)), fof_members);
    const size_t bound_groups = std::min(size_t(std::max(total[0], 0)), fof_groups);
    if (n_groups_out) *n_groups_out = bound_groups;
    if (n_members_out) *n_members_out = bound_members;
    if ((list && bound_groups > group_cap) || ((members || energy) && bound_members > member_cap))
        return fail(h, NBODY_ERR_CAPACITY, std::string(call) + ": buffer too small");
    // only the reported records, members and energies cross to the host
    if (list && bound_groups)
        HIP_TRY(h, hipMemcpyAsync(list, u.out, bound_groups * sizeof(NbodyBoundGroup), hipMemcpyDeviceToHost, h->stream));
    if (members && bound_members)
        HIP_TRY(h, hipMemcpyAsync(members, u.out_members, bound_members * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (energy && bound_members)
        HIP_TRY(h, hipMemcpyAsync(energy, u.out_energy, bound_members * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}
template int bound_groups<float>(NbodyHandle*, const ShardT<float>&, size_t, double, double, double, int, int, NbodyBoundGroup*, size_t,
                                 size_t*, int32_t*, size_t, size_t*, double*);
template int bound_groups<double>(NbodyHandle*, const ShardT<double>&, size_t, double, double, double, int, int, NbodyBoundGroup*, size_t,
                                  size_t*, int32_t*, size_t, size_t*, double*);

}}  // namespace nbody::fof
