// nbody_field.cpp -- nbody_field_at and nbody_tidal_at behind the preparation they share with nbody_potentials: the batches.
#include "nbody_field.h"
#include "nbody_engine.h"

#include <algorithm>

namespace nbody { namespace field {

namespace {

int ensure(NbodyHandle* h, size_t plane_doubles, size_t out_doubles) {
    FieldBufs& f = h->field;
    if (!f.sort_bytes) f.sort_bytes = std::max<size_t>(field_sort_tmp_bytes(kFieldBatch), 256);
    // (each on its own: a call that ran out of memory half way leaves the next one to allocate the rest)
    if (!f.d_xyz) HIP_TRY(h, h->mem.dev(f.d_xyz, kFieldBatch * 3 * sizeof(double)));
    if (!f.d_keys) HIP_TRY(h, h->mem.dev(f.d_keys, 2 * kFieldBatch * sizeof(unsigned long long)));
    if (!f.d_idx) HIP_TRY(h, h->mem.dev(f.d_idx, 2 * kFieldBatch * sizeof(int)));
    if (!f.d_sort_tmp) HIP_TRY(h, h->mem.dev(f.d_sort_tmp, f.sort_bytes));
    // (exactly what is asked for: nbody_field_at alone never holds more than its four per probe)
    HIP_TRY(h, grow_dev(h, f.d_out, f.out_cap, out_doubles, sizeof(double), Grow::exact));
    HIP_TRY(h, grow_dev(h, f.d_planes, f.planes_cap, plane_doubles, sizeof(double), Grow::quarter));
    return NBODY_OK;
}

}  // namespace

int run(NbodyHandle* h, int mode, const PotBodies& b, double g, const double* xyz, size_t n_points, const Out& out, uint64_t counts[2]) {
    FieldBufs& f = h->field;
    PotBufs& p = h->pot;
    const bool tree = mode != NBODY_POTENTIAL_PAIRS;   // (NBODY_POTENTIAL_TREE_QUADRUPOLE: f.quad is set)
    const bool tidal = out.tidal;
    double* const vec = tidal ? out.tidal6 : out.acc;   // the caller's rows of `rows` doubles ...
    double* const phi = tidal ? nullptr : out.phi;      // ... and nbody_field_at's scalars
    const size_t rows = tidal ? 6 : 3;
    const ProbeTerm term = tidal ? (vec ? ProbeTerm::Tidal : ProbeTerm::TidalCount)
                                 : vec && phi ? ProbeTerm::Field : vec ? ProbeTerm::FieldAcc : phi ? ProbeTerm::FieldPhi : ProbeTerm::FieldCount;
    const size_t per = probe_sums(term);   // doubles per plane row and per probe of d_out
    double g_soft = 0.0, theta2 = 0.0, center[3] = {0.0, 0.0, 0.0}, width = 0.0;
    with_bodies(h, [&](const auto& st) {   // the settings and the root box of the handle's store, widened
        g_soft = double(st.g_soft); theta2 = double(st.theta2); width = double(st.width);
        std::copy(st.center, st.center + 3, center);
        return 0;
    });
    const size_t n_bodies = size_t(b.seg_cap) * size_t(b.n_seg);   // (an upper bound is all the slice count needs)
    // once per call: the walk's segments (the force pass drew them from n_points), or the pair kernel's slices
    const size_t first_batch = std::min(n_points, kFieldBatch);
    const int K = tree ? std::max(f.K, 1) : probe_pairs_slices(term, first_batch, n_bodies);
    const bool walk = tree && f.nodes && f.n_nodes > 0;   // (no nodes: an empty world, the field is zero)
    const size_t stride = (std::max<size_t>(first_batch, 1) + 63) / 64 * 64;
    int rc = ensure(h, size_t(K) * stride * per, kFieldBatch * per);
    if (rc) return rc;
    FieldTree ft;
    ft.nodes = f.nodes; ft.K = K; ft.first = f.first; ft.anc = f.anc; ft.n_anc = f.n_anc;
    double* d_vec = vec ? f.d_out : nullptr;
    double* d_phi = phi ? f.d_out + 3 * kFieldBatch : nullptr;
    for (size_t at = 0; at < n_points; at += kFieldBatch) {
        const int n = int(std::min(kFieldBatch, n_points - at));
        HIP_TRY(h, hipMemcpyAsync(f.d_xyz, xyz + 3 * at, size_t(n) * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        const int* idx = nullptr;
        if (tree && !walk) {
            if (!probe_counts_only(term)) HIP_TRY(h, hipMemsetAsync(f.d_out, 0, kFieldBatch * per * sizeof(double), h->stream));
        } else {
            if (!tree) {
                launch_probe_pairs(h->stream, term, b, f.d_xyz, n, K, g_soft * g_soft, f.d_planes, stride);
            } else if (field_sort_probes(h->stream, f.d_xyz, n, b.f64, center, width, f.d_sort_tmp, f.sort_bytes, f.d_keys, f.d_idx, kFieldBatch, &idx) != 0) {
                return fail(h, NBODY_ERR_HIP, std::string(tidal ? "nbody_tidal_at" : "nbody_field_at") + ": rocPRIM call failed");
            } else if (b.f64) {
                nbody64::launch_bh_probe_walk(h->stream, term, ft, f.d_xyz, idx, n, g_soft * g_soft, theta2, f.d_planes, stride, p.d_counts);
            } else if (f.quad && !tidal) {
                launch_bh_field_walk_quad(h->stream, ft, f.quad, f.d_xyz, idx, n, float(g_soft) * float(g_soft), float(theta2), (vec ? 1 : 0) | (phi ? 2 : 0),
                                          reinterpret_cast<double4*>(f.d_planes), stride, p.d_counts);
            } else {
                launch_bh_probe_walk(h->stream, term, ft, f.d_xyz, idx, n, float(g_soft) * float(g_soft), float(theta2), f.d_planes, stride, p.d_counts);
            }
            launch_probe_reduce(h->stream, term, f.d_planes, K, stride, idx, n, g, d_vec, d_phi);
        }
        HIP_TRY(h, hipGetLastError());
        if (vec) HIP_TRY(h, hipMemcpyAsync(vec + rows * at, d_vec, size_t(n) * rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (phi) HIP_TRY(h, hipMemcpyAsync(phi + at, d_phi, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the batch's buffers are reused by the next one)
    }
    if (counts) {
        counts[0] = counts[1] = 0;
        if (tree) {
            HIP_TRY(h, hipMemcpyAsync(p.h_counts, p.d_counts, 2 * NBODY_WALK_COUNTER_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            for (unsigned k = 0; k < NBODY_WALK_COUNTER_SLOTS; ++k) { counts[0] += p.h_counts[2 * k]; counts[1] += p.h_counts[2 * k + 1]; }
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NBODY_OK;
}

}}  // namespace nbody::field
