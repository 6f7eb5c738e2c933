// kernels_poisson.h -- launchers of the grid Poisson solve (kernels_poisson.hip): a radix-2 f64 FFT along each axis of a
// padded complex grid, the Green's-function multiply and the copy between the real and the complex grid.  The arithmetic is
// poisson_grid.h's.  Internal to libnbody_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "poisson_grid.h"

namespace nbody { namespace poisson {

constexpr int kPoissonBlock = 256;
constexpr int kLdsPoints = 4096;        // complex points a block of k_poisson_fft_lds holds at most: one line of the longest axis
constexpr int kLdsPointsSmall = 1024;   // the instance with the smaller LDS image, taken whenever a block's lines fit it
constexpr int kMaxTile = 64;

// how a call transforms (the poisson_lds and poisson_tile knobs)
struct Plan {
    int lds = 1;     // 1: k_poisson_fft_lds; 0: k_poisson_bitrev and one k_poisson_fft_stage launch per stage
    int tile = 16;   // lines per block of the strided passes: the knob brought into 1 .. kMaxTile and down to a power of two
    int code() const { return lds | tile << 1; }
};
Plan make_plan();   // from the knobs of the handle this thread serves

// the lines per block of an axis pass under the LDS plan: `lines` lines of L points, `inner` points between two points of a line
// (inner == 1: the lines lie one after the other and a block takes adjacent ones; else it takes z-adjacent ones)
int lines_per_block(const Plan& p, size_t L, size_t inner, size_t lines);

// The scratch of one call, carved out of one allocation of scratch_bytes.
struct Scratch {
    double* real = nullptr;   // [cells] the caller's mass on its way up, phi on its way down
    Cx* x = nullptr;          // [points] the padded grid
    Cx* k = nullptr;          // [points] Kr (isolated)
    Cx* tw[3] = {nullptr, nullptr, nullptr};       // [len / 2] the twiddles of an axis
    double* K[3] = {nullptr, nullptr, nullptr};    // [n] periodic
    double* D[3] = {nullptr, nullptr, nullptr};    // [n] periodic, deconvolve > 0
};
// own_real == false (nbody_pm.cpp): no room for w.real, which the caller points at a grid that is on the device already
size_t scratch_bytes(const Shape& sh, bool deconvolve, bool own_real = true);
Scratch scratch_layout(void* base, const Shape& sh, bool deconvolve, bool own_real = true);

// k_poisson_load: w.x from w.real, +0.0 in the imaginary parts and in the padding
void launch_load(hipStream_t s, const Shape& sh, const Scratch& w);
// k_poisson_kernel: w.k = Kr
void launch_kernel(hipStream_t s, const Shape& sh, double spacing, double soften, const Scratch& w);
// the lines along z, then y, then x of x (w.x or w.k), under the plan; returns the butterfly launches made
int launch_transform(hipStream_t s, const Shape& sh, const Plan& p, Cx* x, const Scratch& w, bool inverse);
// k_poisson_green: w.x times the periodic Green's function
void launch_green(hipStream_t s, const Shape& sh, double c, bool deconvolve, const Scratch& w);
// k_poisson_mul: w.x = cmul(w.k, w.x)
void launch_mul(hipStream_t s, const Shape& sh, const Scratch& w);
// k_poisson_store: w.real = phi of the nx ny nz corner of w.x
void launch_store(hipStream_t s, const Shape& sh, double g, double inv_points, const Scratch& w);

}}  // namespace nbody::poisson
