// nbody_field.cpp -- nbody_field_at and nbody_tidal_at behind the preparation they share with nbody_potentials: the batches.
#include "nbody_field.h"
#include "nbody_f64.h"

#include <algorithm>

namespace nbody { namespace field {

namespace {

int ensure(NbodyHandle* h, size_t plane_doubles, size_t out_doubles) {
    FieldBufs& f = h->field;
    if (!f.sort_bytes) f.sort_bytes = std::max<size_t>(field_sort_tmp_bytes(kFieldBatch), 256);
    // (each on its own: a call that ran out of memory half way leaves the next one to allocate the rest)
    if (!f.d_xyz) HIP_TRY(h, hipMalloc(&f.d_xyz, kFieldBatch * 3 * sizeof(double)));
    if (!f.d_keys) HIP_TRY(h, hipMalloc(&f.d_keys, 2 * kFieldBatch * sizeof(unsigned long long)));
    if (!f.d_idx) HIP_TRY(h, hipMalloc(&f.d_idx, 2 * kFieldBatch * sizeof(int)));
    if (!f.d_sort_tmp) HIP_TRY(h, hipMalloc(&f.d_sort_tmp, f.sort_bytes));
    if (f.out_cap < out_doubles) {   // (exactly what is asked for: nbody_field_at alone never holds more than its four per probe)
        if (f.d_out) (void)hipFree(f.d_out);
        f.d_out = nullptr; f.out_cap = 0;
        HIP_TRY(h, hipMalloc(&f.d_out, out_doubles * sizeof(double)));
        f.out_cap = out_doubles;
    }
    return grow_dev(h, f.d_planes, f.planes_cap, plane_doubles, sizeof(double));
}

}  // namespace

int run(NbodyHandle* h, int mode, const PotBodies& b, double g, const double* xyz, size_t n_points, const Out& out, uint64_t counts[2]) {
    FieldBufs& f = h->field;
    PotBufs& p = h->pot;
    const bool tree = mode != NBODY_POTENTIAL_PAIRS;   // (NBODY_POTENTIAL_TREE_QUADRUPOLE: f.quad is set)
    const bool tidal = out.tidal;
    const int want = tidal ? (out.tidal6 ? 1 : 0) : (out.acc ? 1 : 0) | (out.phi ? 2 : 0);
    const size_t per = tidal ? 6 : 4;   // doubles per plane row and per probe of d_out
    double g_soft = double(h->g_soft), theta2 = double(h->theta2), center[3] = {double(h->center[0]), double(h->center[1]), double(h->center[2])};
    double width = double(h->width);
    if (b.f64) {
        double g64 = 0.0, dt = 0.0;
        nbody64::get_settings(h, &g64, &g_soft, &dt, &theta2);
        nbody64::get_bounds(h, center, &width);
    }
    const size_t n_bodies = size_t(b.seg_cap) * size_t(b.n_seg);   // (an upper bound is all the slice count needs)
    // once per call: the walk's segments (the force pass drew them from n_points), or the pair kernel's slices
    const size_t first_batch = std::min(n_points, kFieldBatch);
    const int K = tree ? std::max(f.K, 1) : tidal ? tidal_pairs_slices(first_batch, n_bodies) : field_pairs_slices(first_batch, n_bodies);
    const bool walk = tree && f.nodes && f.n_nodes > 0;   // (no nodes: an empty world, the field is zero)
    const size_t stride = (std::max<size_t>(first_batch, 1) + 63) / 64 * 64;
    int rc = ensure(h, size_t(K) * stride * per, kFieldBatch * per);
    if (rc) return rc;
    double4* planes = reinterpret_cast<double4*>(f.d_planes);
    double2* planes6 = reinterpret_cast<double2*>(f.d_planes);   // nbody_tidal_at: rows of kTidalRow double2
    FieldTree ft;
    ft.nodes = f.nodes; ft.K = K; ft.first = f.first; ft.anc = f.anc; ft.n_anc = f.n_anc;
    double* d_acc = out.acc ? f.d_out : nullptr;
    double* d_phi = out.phi ? f.d_out + 3 * kFieldBatch : nullptr;
    double* d_tidal = out.tidal6 ? f.d_out : nullptr;
    for (size_t at = 0; at < n_points; at += kFieldBatch) {
        const int n = int(std::min(kFieldBatch, n_points - at));
        HIP_TRY(h, hipMemcpyAsync(f.d_xyz, xyz + 3 * at, size_t(n) * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        const int* idx = nullptr;
        if (tree && !walk) {
            if (want) HIP_TRY(h, hipMemsetAsync(f.d_out, 0, kFieldBatch * per * sizeof(double), h->stream));
        } else if (tree) {
            if (field_sort_probes(h->stream, f.d_xyz, n, b.f64, center, width, f.d_sort_tmp, f.sort_bytes, f.d_keys, f.d_idx, kFieldBatch, &idx) != 0)
                return fail(h, NBODY_ERR_HIP, std::string(tidal ? "nbody_tidal_at" : "nbody_field_at") + ": rocPRIM call failed");
            if (tidal) {
                if (b.f64) nbody64::launch_bh_tidal_walk(h->stream, ft, f.d_xyz, idx, n, g_soft * g_soft, theta2, want, planes6, stride, p.d_counts);
                else launch_bh_tidal_walk(h->stream, ft, f.d_xyz, idx, n, h->g_soft * h->g_soft, h->theta2, want, planes6, stride, p.d_counts);
                launch_tidal_reduce(h->stream, planes6, K, stride, idx, n, g, d_tidal);
            } else {
                if (b.f64) nbody64::launch_bh_field_walk(h->stream, ft, f.d_xyz, idx, n, g_soft * g_soft, theta2, want, planes, stride, p.d_counts);
                else if (f.quad) launch_bh_field_walk_quad(h->stream, ft, f.quad, f.d_xyz, idx, n, h->g_soft * h->g_soft, h->theta2, want, planes, stride, p.d_counts);
                else launch_bh_field_walk(h->stream, ft, f.d_xyz, idx, n, h->g_soft * h->g_soft, h->theta2, want, planes, stride, p.d_counts);
                launch_field_reduce(h->stream, planes, K, stride, idx, n, g, d_acc, d_phi);
            }
        } else if (want && tidal) {
            launch_tidal_pairs(h->stream, b, f.d_xyz, n, K, g_soft * g_soft, planes6, stride);
            launch_tidal_reduce(h->stream, planes6, K, stride, nullptr, n, g, d_tidal);
        } else if (want) {
            launch_field_pairs(h->stream, b, f.d_xyz, n, K, g_soft * g_soft, planes, stride);
            launch_field_reduce(h->stream, planes, K, stride, nullptr, n, g, d_acc, d_phi);
        }
        HIP_TRY(h, hipGetLastError());
        if (out.acc) HIP_TRY(h, hipMemcpyAsync(out.acc + 3 * at, d_acc, size_t(n) * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (out.phi) HIP_TRY(h, hipMemcpyAsync(out.phi + at, d_phi, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (out.tidal6) HIP_TRY(h, hipMemcpyAsync(out.tidal6 + 6 * at, d_tidal, size_t(n) * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
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
