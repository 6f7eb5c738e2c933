// kernels_pm.h -- launchers of the particle-mesh field (kernels_pm.hip): the one scratch of a call, which holds the pieces of the
// deposit, the Poisson solve and the gather with the grid shared among them, and k_pm_gather, which reads acc and phi off the
// resident grid in one pass.  The arithmetic is deposit_grid.h's, poisson_grid.h's and sample_grid.h's.  Internal to
// libnbody_hip.so.
#pragma once
#include "kernels_deposit.h"
#include "kernels_poisson.h"
#include "kernels_sample.h"
#include "pm_grid.h"

namespace nbody { namespace pm {

// how a call runs (the pm_gather and pm_share_sort knobs)
struct Plan {
    int gather = 1;       // 1: k_pm_gather; 0: two k_sample launches, gradient then value, and k_pm_negate
    int share_sort = 1;   // 1: at the bodies one home-cell order serves k_deposit and the gather (both stages' sorts on); 0: each its own
    int code() const { return gather | share_sort << 1; }
};
Plan make_plan();   // from the knobs of the handle this thread serves

// the plans of the stages, from the same knobs
struct Plans {
    Plan pm;
    deposit::Plan dep;
    poisson::Plan poi;
    sample::Plan grad, value;   // the gradient pass (pregrad honoured where pm.gather == 0) and the value pass
    bool shared = false;        // one order serves both stages in this call
};
Plans make_plans(int gradient_op, size_t cells, bool at_bodies);

// The scratch of one call over n_bodies body rows and n_rows point rows (the bodies themselves: n_rows == n_bodies), carved out
// of ONE allocation of scratch_bytes.  dep.acc, poi.real and smp.grid are one block: int64 sums, then the mass in doubles,
// then phi.
struct Scratch {
    deposit::Scratch dep;
    poisson::Scratch poi;
    sample::Scratch smp;           // out: the gradient rows, negated in place where pm.gather == 0, else acc as it is returned
    double* phi = nullptr;         // [n_rows]
    sample::Words* value_words = nullptr;   // pm.gather == 0: the value pass's words
    uint8_t* value_cls = nullptr;           // pm.gather == 0: [n_rows] the value pass's classes, which nobody reads
};
size_t scratch_bytes(size_t n_bodies, size_t n_rows, const deposit::Grid& g, const poisson::Shape& sh, bool deconvolve, int gradient_op,
                     const Plans& p);
Scratch scratch_layout(void* base, size_t n_bodies, size_t n_rows, const deposit::Grid& g, const poisson::Shape& sh, bool deconvolve,
                       int gradient_op, const Plans& p);

// w.smp.words zeroed; k_pm_gather over the n rows of w.smp.xyz, of which the first *count are live (count == nullptr: all n):
// w.smp.out = acc, w.phi (with_phi), w.smp.cls.  rows: the n rows in home-cell order, or null: in row order.
void launch_gather(hipStream_t s, const int* count, int n, const deposit::Grid& g, int gradient_op, bool with_phi, const int* rows, const Scratch& w);

// k_pm_negate: rows[i] = 0.0 - rows[i] over the first 3 * live doubles
void launch_negate(hipStream_t s, const int* count, int n, double* rows);

}}  // namespace nbody::pm
