// nbody_cells.h -- the host side of the cell-list pair search (include/nbody_hip.h, "pair search"): what a fixed-radius call
// (nbody_fof.cpp find_groups, nbody_pairs.cpp find_contacts, nbody_within.cpp Lists::count) does before its pair pass when the handle is in
// NBODY_SEARCH_CELLS, and the record it leaves behind.  nbody_knn.cpp Rows::run does the same for the length of its radius hint.
// Internal to libnbody_hip.so.
#pragma once
#include "nbody_handle.h"
#include "kernels_cells.h"

namespace nbody { namespace cells {

// One search: its scratch (through the handle's registry, freed with this object, i.e. inside the call), and whether the grid
// was drawn.  on == false -- the handle is in NBODY_SEARCH_ALL_PAIRS, no body is gridded or the grid is not usable -- means
// the caller runs its all-pairs pass; then `scratch` was never allocated (`bounds`, 56 bytes, only under NBODY_SEARCH_CELLS).
struct Search {
    explicit Search(HandleMem& mem) : bounds(mem), scratch(mem) {}
    ScratchDev bounds;    // the BoundsWords, needed before the decision
    ScratchDev scratch;   // everything else (w), once the grid is known to be usable
    CellScratch w;
    bool on = false;
    int n_gridded = 0;
};

// Under NBODY_SEARCH_CELLS: the bounds of sh's live, gridded bodies (one read-back and synchronisation), the grid for
// `length`, and -- when it is usable -- the bodies in cell order (s->on).  Nothing of the handle's is written.
template <class F>
int prepare(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double length, const char* call, Search* s);

// The call's one synchronisation after its pair pass: enqueues the copy of the search's counters into *c (s.on) and
// synchronises the stream -- also when the copy could not be enqueued, so no copy into the caller's frame outlives this call;
// the caller enqueues its own read-backs before it.  Then the record behind nbody_pair_search_stats:
// {1, gridded, occupied, candidates}, or zeros for an all-pairs pass.
int fetch_counters(NbodyHandle* h, const Search& s, Counters* c);
void record(NbodyHandle* h, const Search& s, const Counters& c);

}}  // namespace nbody::cells
