// nbody_deposit.cpp -- nbody_deposit and nbody_host_deposit (include/nbody_hip.h, "grid deposit"): the check of a spec, the
// scratch of a call, the launches of kernels_deposit.hip, the copy of the grid and of the four counts, and the host twin.
#include "nbody_deposit.h"

#include <algorithm>

namespace nbody { namespace deposit {

template <class F>
int deposit(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, double* grid, uint64_t* counts) {
    const Grid g = grid_of(spec);
    const size_t cells = cells_of(g);
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!n_upper) {   // no body: every cell +0.0
        if (grid) std::fill(grid, grid + cells, 0.0);
        return NBODY_OK;
    }
    const Plan plan = make_plan();
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, cells, grid != nullptr, plan.sort != 0)));
    const Scratch w = scratch_layout(scratch.get(), n_upper, cells, grid != nullptr, plan.sort != 0);
    launch_q<F>(h->stream, sh, int(n_upper), g, spec.quantity, w);
    Enqueued st;
    if (grid) st.prim(launch_deposit<F>(h->stream, sh, int(n_upper), g, plan, w));
    Words words{};
    st.last();
    if (st.ok()) st.hip(hipMemcpyAsync(&words, w.words, sizeof(Words), hipMemcpyDeviceToHost, h->stream));
    if (st.ok() && grid) st.hip(hipMemcpyAsync(grid, w.acc, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (const int rc = st.finish(h, "nbody_deposit")) return rc;
    if (counts) std::copy(words.counts, words.counts + 4, counts);
    h->deposit_last[0] = 1;
    h->deposit_last[1] = uint64_t(plan.code());
    h->deposit_last[2] = words.terms;
    h->deposit_last[3] = words.atomics;
    return NBODY_OK;
}
template int deposit<float>(NbodyHandle*, const ShardT<float>&, size_t, const NbodyGridSpec&, double*, uint64_t*);
template int deposit<double>(NbodyHandle*, const ShardT<double>&, size_t, const NbodyGridSpec&, double*, uint64_t*);

}}  // namespace nbody::deposit
