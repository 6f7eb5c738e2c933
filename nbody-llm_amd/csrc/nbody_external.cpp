// nbody_external.cpp -- the static external field (include/nbody_hip.h, "external field"): what a handle holds, the launch
// after a force pass, the f64 potentials and probes, and the host-only evaluation of external_field.h's expressions.
#include "nbody_external.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace nbody { namespace ext {

const char* refusal(const NbodyHandle* h) {
    if (h->let || h->cfg.shard_mode != NBODY_SHARD_INDEX) return "NBODY_SHARD_SPATIAL handles take no external field (out of scope)";
    if (h->cfg.world_size != 1) return "handles of a multi-rank world take no external field (out of scope)";
    return nullptr;
}

namespace {

template <class T>
std::string invalid_as(const NbodyExternalComponent* comps, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const NbodyExternalComponent& c = comps[i];
        const std::string at = "component " + std::to_string(i) + ": ";
        if (c.kind < NBODY_EXT_PLUMMER || c.kind > NBODY_EXT_LOGARITHMIC) return at + "unknown kind";
        if (c.reserved != 0) return at + "reserved must be 0";
        T p[4];
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(T(c.center[k]))) return at + "non-finite center";
        for (int k = 0; k < 4; ++k) {
            p[k] = T(c.p[k]);
            if (!std::isfinite(p[k])) return at + "non-finite parameter";
        }
        switch (c.kind) {
            case NBODY_EXT_PLUMMER:
                if (!(p[1] >= T(0))) return at + "NBODY_EXT_PLUMMER needs b >= 0";
                break;
            case NBODY_EXT_HERNQUIST:
                if (!(p[1] > T(0))) return at + "NBODY_EXT_HERNQUIST needs a > 0";
                break;
            case NBODY_EXT_MIYAMOTO_NAGAI:
                if (!(p[1] >= T(0)) || !(p[2] > T(0))) return at + "NBODY_EXT_MIYAMOTO_NAGAI needs a >= 0 and b > 0";
                break;
            default:
                if (!(p[1] > T(0)) || !(p[2] > T(0)) || !(p[3] > T(0))) return at + "NBODY_EXT_LOGARITHMIC needs rc > 0, qy > 0 and qz > 0";
                break;
        }
    }
    return std::string();
}

FieldT<double> as_given(const NbodyExternalComponent* comps, size_t n) {
    ExternalField e;
    e.n = int(n);
    std::copy(comps, comps + n, e.given);
    return rounded<double>(e);
}

}  // namespace

std::string invalid(const NbodyExternalComponent* comps, size_t n, bool f32) {
    if (n > NBODY_EXTERNAL_MAX) return "more than NBODY_EXTERNAL_MAX components";
    if (n && !comps) return "comps is NULL";
    std::string why = invalid_as<double>(comps, n);
    if (why.empty() && f32) {
        why = invalid_as<float>(comps, n);
        if (!why.empty()) why += " (as rounded to f32, the handle's precision)";
    }
    return why;
}

template <class F>
FieldT<F> rounded(const ExternalField& e) {
    FieldT<F> f{};
    f.n = e.n;
    for (int i = 0; i < e.n; ++i) {
        f.c[i].kind = e.given[i].kind;
        for (int k = 0; k < 3; ++k) f.c[i].c[k] = F(e.given[i].center[k]);
        for (int k = 0; k < 4; ++k) f.c[i].p[k] = F(e.given[i].p[k]);
    }
    return f;
}
template FieldT<float> rounded<float>(const ExternalField&);
template FieldT<double> rounded<double>(const ExternalField&);

template <class F>
int add(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, F g, const F* kick_dt, bool count_step) {
    launch_ext_add<F>(h->stream, sh, int(n_upper), rounded<F>(h->ext), g, kick_dt, count_step);
    HIP_TRY(h, hipGetLastError());
    return NBODY_OK;
}
template int add<float>(NbodyHandle*, const ShardT<float>&, size_t, float, const float*, bool);
template int add<double>(NbodyHandle*, const ShardT<double>&, size_t, double, const double*, bool);

// scratch of its own, allocated and freed inside the call: nothing of the handle's is written
template <class F>
int potentials(NbodyHandle* h, const ShardT<F>& sh, size_t n, double g, double* phi, double* energy) {
    if (energy) *energy = 0.0;
    const size_t blocks = size_t(blocks_for(int(n)));
    if (!blocks) return NBODY_OK;
    ScratchDev scratch(h->mem);   // [n] potentials | [blocks] block sums
    HIP_TRY(h, scratch.alloc((n + blocks) * sizeof(double)));
    double* d = scratch.get<double>();
    launch_ext_phi<F>(h->stream, sh, int(n), rounded<double>(h->ext), g, phi ? d : nullptr, d + n);
    std::vector<double> part(blocks);
    HIP_TRY(h, hipGetLastError());
    if (phi) HIP_TRY(h, hipMemcpyAsync(phi, d, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(part.data(), d + n, blocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double sum = 0.0;
    for (size_t b = 0; b < blocks; ++b) sum += part[b];   // blocks in ascending order
    if (energy) *energy = sum;
    return NBODY_OK;
}
template int potentials<float>(NbodyHandle*, const ShardT<float>&, size_t, double, double*, double*);
template int potentials<double>(NbodyHandle*, const ShardT<double>&, size_t, double, double*, double*);

int at(NbodyHandle* h, double g, const double* xyz, size_t n_points, double* acc, double* phi) {
    if (!n_points || (!acc && !phi)) return NBODY_OK;
    const size_t batch = std::min(n_points, kFieldBatch);
    ScratchDev scratch(h->mem);   // [batch][3] points | [batch][3] accelerations | [batch] potentials
    HIP_TRY(h, scratch.alloc(batch * 7 * sizeof(double)));
    double* d = scratch.get<double>();
    double* d_acc = d + 3 * batch;
    double* d_phi = d + 6 * batch;
    const FieldT<double> f = rounded<double>(h->ext);
    for (size_t at0 = 0; at0 < n_points; at0 += batch) {
        const size_t n = std::min(batch, n_points - at0);
        HIP_TRY(h, hipMemcpyAsync(d, xyz + 3 * at0, n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_ext_at(h->stream, d, int(n), f, g, acc ? d_acc : nullptr, phi ? d_phi : nullptr);
        HIP_TRY(h, hipGetLastError());
        if (acc) HIP_TRY(h, hipMemcpyAsync(acc + 3 * at0, d_acc, n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (phi) HIP_TRY(h, hipMemcpyAsync(phi + at0, d_phi, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the batch's buffers are reused by the next one)
    }
    return NBODY_OK;
}

}}  // namespace nbody::ext

extern "C" int nbody_host_external_eval(const NbodyExternalComponent* comps, size_t n, double g, const double* xyz, size_t n_points,
                                        double* acc, double* phi) {
    const std::string why = nbody::ext::invalid(comps, n, false);
    if (!why.empty()) return fail(nullptr, NBODY_ERR_INVALID, "nbody_host_external_eval: " + why);
    if (!std::isfinite(g)) return fail(nullptr, NBODY_ERR_INVALID, "nbody_host_external_eval: non-finite g");
    if (!xyz && n_points) return fail(nullptr, NBODY_ERR_INVALID, "nbody_host_external_eval: xyz is NULL");
    const nbody::ext::FieldT<double> f = nbody::ext::as_given(comps, n);
    for (size_t k = 0; k < n_points; ++k)
        nbody::ext::eval_point(f, g, xyz + 3 * k, acc ? acc + 3 * k : nullptr, phi ? phi + k : nullptr);
    return NBODY_OK;
}
