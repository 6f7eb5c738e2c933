// nbody_cells.cpp -- the host side of the cell-list pair search (nbody_cells.h).
#include "nbody_cells.h"

#include <string>

namespace nbody { namespace cells {

template <class F>
int prepare(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double length, const char* call, Search* s) {
    s->on = false;
    if (h->search.mode != NBODY_SEARCH_CELLS || !n_upper) return NBODY_OK;
    HIP_TRY(h, s->bounds.alloc(sizeof(BoundsWords)));
    launch_bounds<F>(h->stream, sh, int(n_upper), s->bounds.get<BoundsWords>());
    BoundsWords words{};
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(&words, s->bounds.get(), sizeof(words), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double lo[3], hi[3];
    const size_t gridded = std::min(bounds_of(words, lo, hi), n_upper);
    const Grid g = make_grid(lo, hi, gridded > 0, length);
    if (!gridded || !g.usable) return NBODY_OK;   // the all-pairs pass: the scratch of a search is never allocated
    HIP_TRY(h, s->scratch.alloc(scratch_bytes(n_upper)));
    s->w = scratch_layout(s->scratch.get(), n_upper);
    if (launch_order<F>(h->stream, sh, int(n_upper), int(gridded), g, s->w) != 0)
        return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
    s->n_gridded = int(gridded);
    s->on = true;
    return NBODY_OK;
}
template int prepare<float>(NbodyHandle*, const ShardT<float>&, size_t, double, const char*, Search*);
template int prepare<double>(NbodyHandle*, const ShardT<double>&, size_t, double, const char*, Search*);

int fetch_counters(NbodyHandle* h, const Search& s, Counters* c) {
    *c = Counters{};
    const hipError_t counters_copy = s.on ? hipMemcpyAsync(c, s.w.counters, sizeof(Counters), hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    const hipError_t stream_sync = hipStreamSynchronize(h->stream);   // whether or not the copy was enqueued: *c may be a local
    HIP_TRY(h, counters_copy);
    HIP_TRY(h, stream_sync);
    return NBODY_OK;
}

void record(NbodyHandle* h, const Search& s, const Counters& c) {
    h->search.last[0] = s.on ? 1 : 0;
    h->search.last[1] = s.on ? uint64_t(s.n_gridded) : 0;
    h->search.last[2] = s.on ? c.occupied : 0;
    h->search.last[3] = s.on ? c.candidates : 0;
}

}}  // namespace nbody::cells
