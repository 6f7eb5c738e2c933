// kernels_field.h -- launchers behind nbody_field_at and nbody_tidal_at (internal to libnbody_hip.so): a quantity of all bodies
// at caller-chosen points.  Probes arrive as f64 triples and are rounded once to the handle's precision.  The quantity is a
// Term (probe_term.h): every kernel leaves the Term's sums -- field {sum m d / s^3, sum m / s} (d = x_j - x, s = sqrt(|d|^2 +
// eps2)), tidal {xx, xy, xz, yy, yz, zz} -- per (segment or slice, probe) in planes of rows of probe_sums(term) doubles, each row
// written once; the reduce adds them in plane order, multiplies by g and scatters to the caller's order.
#pragma once
#include "kernels_pot.h"

namespace nbody {

// what a call sums (FieldAcc / FieldPhi: the vector / the scalar part alone; ...Count: nothing, the walk only counts)
enum class ProbeTerm { Field, FieldAcc, FieldPhi, FieldCount, Tidal, TidalCount };
constexpr bool probe_tidal(ProbeTerm t) { return t == ProbeTerm::Tidal || t == ProbeTerm::TidalCount; }
constexpr bool probe_counts_only(ProbeTerm t) { return t == ProbeTerm::FieldCount || t == ProbeTerm::TidalCount; }
constexpr size_t probe_sums(ProbeTerm t) { return probe_tidal(t) ? 6 : 4; }   // doubles per plane row

// the tree a probe call walks: the force pass's nodes and split points (FieldBufs)
struct FieldTree {
    const void* nodes = nullptr;   // NodeDev (f32 handles) or Node64 (f64)
    int K = 1;
    const int* first = nullptr;
    const int* anc = nullptr;
    const int* n_anc = nullptr;
};

// Morton keys of n probes in the handle's box (the device build's key layout; outside the box the orthant descent saturates,
// NaN compares false), then {key, place in the batch} sorted by key: idx [n] = the batch's probes in tree order
size_t field_sort_tmp_bytes(size_t n_cap);
int field_sort_probes(hipStream_t s, const double* xyz, int n, int f64, const double center[3], double width, void* tmp, size_t tmp_bytes,
                      unsigned long long* keys /* [2][n_cap] */, int* idx /* [2][n_cap] */, size_t n_cap, const int** sorted_idx);

// NBODY_POTENTIAL_TREE: one probe per lane in idx order over the node-range split, the potential walk's tests (DIRECT rule);
// terms in the handle's precision, f64 sums.  One traversal whatever the term: {accepted, visited} do not depend on it
void launch_bh_probe_walk(hipStream_t s, ProbeTerm term, const FieldTree& t, const double* xyz, const int* idx, int n, float eps2, float theta2,
                          double* planes, size_t stride, unsigned long long* counters);
}  // namespace nbody
namespace nbody64 {
void launch_bh_probe_walk(hipStream_t s, nbody::ProbeTerm term, const nbody::FieldTree& t, const double* xyz, const int* idx, int n, double eps2,
                          double theta2, double* planes, size_t stride, unsigned long long* counters);
}
namespace nbody {

// NBODY_POTENTIAL_PAIRS: every live body of every segment, one-sided, in f64; K slices of the concatenated body list.  All of a
// quantity's sums are formed whichever the caller asked for
void launch_probe_pairs(hipStream_t s, ProbeTerm term, const PotBodies& b, const double* xyz, int n, int K, double eps2, double* planes, size_t stride);
// slices for a batch of n probes against n_bodies bodies, so that a few thousand probes still fill the chip
int probe_pairs_slices(ProbeTerm term, size_t n, size_t n_bodies);

// planes added in plane order, at place idx[t] (idx == nullptr: t).  Field: acc [n][3] = +g sum, phi [n] = -g sum, either may be
// null; tidal: acc [n][6] = g sum
void launch_probe_reduce(hipStream_t s, ProbeTerm term, const double* planes, int K, size_t stride, const int* idx, int n, double g, double* acc,
                         double* phi);

}  // namespace nbody
