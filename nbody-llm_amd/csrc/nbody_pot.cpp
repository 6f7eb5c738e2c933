// nbody_pot.cpp -- what nbody_potentials and nbody_energy_world do alike on handles of either dtype: their buffers, the
// pair kernels' plan, the read-back of the per-body sums and counters, the energy partials and their exchange.
#include "nbody_pot.h"

#include <algorithm>
#include <vector>

namespace nbody { namespace pot {

int begin(NbodyHandle* h, size_t bodies) {
    PotBufs& p = h->pot;
    HIP_TRY(h, grow_dev(h, p.d_sum, p.sum_cap, std::max<size_t>(bodies, 1), sizeof(double), Grow::quarter));
    const size_t cb = 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long);
    if (!p.d_counts) {
        HIP_TRY(h, h->mem.dev(p.d_counts, cb));
        HIP_TRY(h, h->mem.pin(p.h_counts, cb));
    }
    HIP_TRY(h, hipMemsetAsync(p.d_counts, 0, cb, h->stream));
    return NBODY_OK;
}

int ensure_planes(NbodyHandle* h, size_t doubles) {
    HIP_TRY(h, grow_dev(h, h->pot.d_planes, h->pot.planes_cap, doubles, sizeof(double), Grow::quarter));
    return NBODY_OK;
}

int pairs(NbodyHandle* h, const PotBodies& b, size_t n, size_t n_remote, double eps2) {
    if (n == 0) return NBODY_OK;
    const nbody64::Bf64Plan plan = nbody64::make_bf64_plan(int(n), int(std::min<size_t>(n_remote, 0x7fffffff)), b.n_seg);
    int rc = ensure_planes(h, size_t(plan.n_planes) * plan.n_pad);
    if (rc) return rc;
    launch_pot_pairs(h->stream, b, plan, h->pot.d_planes, eps2, int(n), h->pot.d_sum);
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}

int download(NbodyHandle* h, size_t n, double g, double* phi, size_t cap, size_t* n_out, uint64_t counts[2]) {
    PotBufs& p = h->pot;
    if (n_out) *n_out = n;
    if (counts) {
        HIP_TRY(h, hipMemcpyAsync(p.h_counts, p.d_counts, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        counts[0] = counts[1] = 0;
        for (unsigned k = 0; k < NBODY_WALK_COUNTER_SLOTS; ++k) { counts[0] += p.h_counts[2 * k]; counts[1] += p.h_counts[2 * k + 1]; }
    }
    if (!phi) { HIP_TRY(h, hipStreamSynchronize(h->stream)); return NBODY_OK; }   // (count only)
    if (n > cap) return fail(h, NBODY_ERR_CAPACITY, "nbody_potentials: buffer too small");
    if (n) HIP_TRY(h, hipMemcpyAsync(phi, p.d_sum, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i) phi[i] = -g * phi[i];
    return NBODY_OK;
}

int energy(NbodyHandle* h, const PotBodies& b, size_t n, double g, double* kinetic, double* potential) {
    PotBufs& p = h->pot;
    const size_t blocks = (n + 255) / 256;
    double mine[2] = {0.0, 0.0};
    if (blocks) {
        HIP_TRY(h, grow_dev(h, p.d_part, p.part_blocks, blocks, 2 * sizeof(double), Grow::quarter));
        launch_pot_energy(h->stream, b, p.d_sum, int(n), p.d_part);
        HIP_TRY(h, hipGetLastError());
        std::vector<double> part(blocks * 2);
        HIP_TRY(h, hipMemcpyAsync(part.data(), p.d_part, blocks * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < blocks; ++k) { mine[0] += part[2 * k]; mine[1] += part[2 * k + 1]; }
    } else {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    mine[1] *= -0.5 * g;   // 1/2 sum m_i phi_i
    double ke = mine[0], pe = mine[1];
    if (b.world > 1) {
        std::vector<double> all(size_t(b.world) * 2);
        TP_TRY(h, h->tp->host_all_gather(mine, all.data(), sizeof(mine)));
        ke = pe = 0.0;
        for (int r = 0; r < b.world; ++r) { ke += all[2 * size_t(r)]; pe += all[2 * size_t(r) + 1]; }   // rank order: the same on every rank
    }
    if (kinetic) *kinetic = ke;
    if (potential) *potential = pe;
    return NBODY_OK;
}

}}  // namespace nbody::pot
