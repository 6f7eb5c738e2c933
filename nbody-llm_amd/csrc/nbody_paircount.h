// nbody_paircount.h -- the binned pair-separation counts behind include/nbody_hip.h ("pair-separation counts"): internal entry
// points.
#pragma once
#include "nbody_handle.h"
#include "kernels_paircount.h"

#include <string>
#include <vector>

namespace nbody { namespace paircount {

// E2[b] = edges[b] * edges[b], each rounded once, into *e2 -- or why the edges are not valid (empty: they are): n_bins outside
// 1 .. NBODY_PAIR_COUNT_MAX_BINS, edges NULL, an edge that is not finite, edges[0] < 0, squares that are not finite or do not
// strictly ascend
std::string squared_edges(const double* edges, int n_bins, std::vector<double>* e2);

// The callers have bound the device, refused the handles nbody_moments refuses (diag::refusal), confirmed enqueued steps and
// checked the arguments; e2 holds the n_bins + 1 squared edges.  n_upper >= the live count of sh (the host's view, which no
// call refreshes): the launches are sized from it and read the live count on the device.  Scratch is allocated and freed
// inside the call; nothing of the handle's is written but -- pair_counts only -- the record behind nbody_pair_search_stats.
// length: |edges[n_bins]|, what a grid is drawn for.  outside may be null.
template <class F>
int pair_counts(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const std::vector<double>& e2, double length, uint64_t* counts,
                uint64_t* outside);
template <class F>
int pair_counts_at(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const double* points, size_t m, const std::vector<double>& e2,
                   uint64_t* counts, uint64_t* outside);

}}  // namespace nbody::paircount
