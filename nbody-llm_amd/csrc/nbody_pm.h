// nbody_pm.h -- the particle-mesh field behind include/nbody_hip.h ("particle-mesh field"): internal entry points.
#pragma once
#include "nbody_handle.h"
#include "kernels_pm.h"

namespace nbody { namespace pm {

// (call_refusal and the host call are pm_grid.h's)

// The caller has bound the device, refused the handles nbody_deposit refuses, confirmed enqueued steps and checked the call
// (pm_grid.h call_refusal).  n_upper >= the live count of sh (the host's view, which no call refreshes): the launches are sized
// from it and read the live count on the device.  Scratch is one allocation, freed inside the call; nothing of the handle's is
// written but the record behind nbody_pm_field_stats.  phi, cls, n_out and counts may be null.
template <class F>
int at_bodies(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, double* acc, double* phi,
              uint8_t* cls, size_t cap, size_t* n_out, uint64_t* counts);

// the same at n_points caller points: the bodies are deposited and the grid is solved once, the points go by in batches
template <class F>
int at_points(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, const double* xyz,
              size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts);

// ---- the stages of a call, for a caller that keeps the scratch between calls (nbody_mesh.cpp)

// what a call holds on the host until its last synchronisation (the tables are read by copies that are only enqueued)
struct Call {
    deposit::Grid g;
    poisson::Shape shape;
    poisson::Tables tables;
    Plans plans;
    bool deconvolve;
    int op;
    bool split;   // r_split > 0 (nbody_p3m.cpp): the tables' D carries the Gaussian split, and `deconvolve` is set with it
    Call(const NbodyGridSpec& spec, const NbodyPmSpec& pm, bool bodies, double r_split = 0.0)
        : g(deposit::grid_of(spec)), shape(poisson::shape_of(spec)), tables(poisson::tables_of(spec, pm.poisson, shape, r_split)),
          plans(make_plans(pm.gradient, deposit::cells_of(g), bodies)),
          deconvolve(shape.periodic && (pm.poisson.deconvolve > 0 || r_split > 0.0)), op(pm.gradient), split(shape.periodic && r_split > 0.0) {}
};

// what the stages count as they enqueue; every stage enqueues against st (nbody_handle.h Enqueued) and does nothing once it is not ok
struct Tally { uint64_t sorts = 0, transforms = 0; };   // radix sorts, 3-D transforms

// shared: one order for both stages -- the sampler's keys, which depend on the position alone -- over the n rows
// of w.smp.xyz; returns it (w.smp.rows + n), or null when not shared
const int* enqueue_shared_order(NbodyHandle* h, const Call& c, const int* count, size_t n, bool shared, const Scratch& w, Enqueued& st, Tally& tally);

// The deposit of the n_upper rows of sh and the solve: w.smp.grid (the deposit's sums, the Poisson stage's real) holds phi, and
// under sample_pregrad the difference grids follow.  ordered_rows: the bodies in home-cell order, made already, or null.
// held: poisson::enqueue's.
template <class F>
void enqueue_grid(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const NbodyGridSpec& spec, const NbodyPmSpec& pm, const Call& c,
                  const Scratch& w, const int* ordered_rows, Enqueued& st, Tally& tally, int held = 0);

// One pass over the n rows of w.smp.xyz (count: the live rows' word on the device, or null: all n) against the resident grid:
// w.smp.out = acc, w.phi (with_phi), w.smp.cls.  ordered: w.smp.rows + n holds these rows' order already.
void enqueue_rows(NbodyHandle* h, const Call& c, const int* count, size_t n, bool with_phi, bool ordered, const Scratch& w, Enqueued& st, Tally& tally);

// what one pass over rows brings down
struct Down {
    deposit::Words dep{};
    sample::Words rows{}, value{};
};
// the copies of a pass's first `copy` rows (acc, phi and cls, each where not null) and of its words
void enqueue_down(NbodyHandle* h, Enqueued& st, const Call& c, const Scratch& w, size_t copy, double* acc, double* phi, uint8_t* cls, Down* down);

}}  // namespace nbody::pm
