// simulation.hpp -- C++ mirror of the reference's `Simulation` trait (src/shared.rs:80-97) over
// the C ABI of include/nbody_hip.h.  The reference's host language is Rust; this image has no Rust
// toolchain, so the host side above the ABI is restated in C++ with the trait's method names,
// argument meaning and ownership rules (the Rust shim itself is nbody-llm_amd/rust/, untested).
//
//   nbody::PointParticleT<F>      = shared.rs:151-158 (#[repr(C)]; F = float: 40 bytes, F = double: 80 bytes --
//                                   the reference's trait is generic over Float and its driver runs f64)
//   nbody::SimulationSettings     = shared.rs:61-78
//   nbody::Bounds                 = shared.rs:216-243 (center, width)
//   nbody::Simulation             = shared.rs:80-97   (abstract)
//   nbody::IntegratorT            = shared.rs:99-104  (the trait's `I`; LeapFrogIntegratorT = shared.rs:106-149)
//   nbody::BruteForceSimulation   = manual/brute_force.rs:11-103
//   nbody::BarnesHutSimulation    = manual/barnes_hut.rs:93-285
//
// Differences from the Rust trait, all forced by the device boundary:
//   - get_points() returns a const reference to a host vector that is refreshed lazily (one D2H
//     copy when the device state is newer), the same trick the Rust shim plays with UnsafeCell;
//   - settings_mut() hands out a reference and the new values are pushed before the next step;
//   - errors: the reference's signatures are infallible (it panics); here a failed ABI call throws
//     nbody::Error carrying the ABI's code and message.
#pragma once
#include <array>
#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nbody_hip.h"

namespace nbody {

template <class F>
struct PointParticleT {  // PointParticle<F, 3>
    F position[3];
    F velocity[3];
    F acceleration[3];
    F mass;
};
using PointParticle = PointParticleT<float>;
using PointParticle64 = PointParticleT<double>;
static_assert(sizeof(PointParticle) == 40 && sizeof(PointParticle64) == 80, "PointParticle must match the reference's #[repr(C)] layout");

template <class F>
struct SimulationSettingsT {  // defaults: shared.rs:69-78
    F g = F(1.0);
    F g_soft = F(0.0);
    F dt = F(1e-3);
    F theta2 = F(0.5);
};
using SimulationSettings = SimulationSettingsT<float>;

template <class F>
struct BoundsT {  // Bounds::new(center, width)
    std::array<F, 3> center{F(0), F(0), F(0)};
    F width = F(1);
};
using Bounds = BoundsT<float>;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

namespace abi {  // the f32 / f64 forms of the entry points that carry scalars
inline int set_settings(NbodyHandle* h, float g, float e, float dt, float t2) { return nbody_set_settings(h, g, e, dt, t2); }
inline int set_settings(NbodyHandle* h, double g, double e, double dt, double t2) { return nbody_set_settings_f64(h, g, e, dt, t2); }
inline int set_bounds(NbodyHandle* h, const float* c, float w) { return nbody_set_bounds(h, c, w); }
inline int set_bounds(NbodyHandle* h, const double* c, double w) { return nbody_set_bounds_f64(h, c, w); }
inline int step_by(NbodyHandle* h, float dt) { return nbody_step_by(h, dt); }
inline int step_by(NbodyHandle* h, double dt) { return nbody_step_by_f64(h, dt); }
inline int elapsed(const NbodyHandle* h, float* t) { return nbody_elapsed(h, t); }
inline int elapsed(const NbodyHandle* h, double* t) { return nbody_elapsed_f64(h, t); }
template <class F> constexpr int dtype_of() { return sizeof(F) == 8 ? NBODY_F64 : NBODY_F32; }
}  // namespace abi

// The reference's `Integrator<F, D, P>` (shared.rs:99-104): the trait is generic over it.  The device integrates with the
// reference's LeapFrogIntegrator itself (kernels K1 / K3: the only integrator the reference ships, and the fast path).
// Any other integrator runs on the host through SimulationT::step_by_with: the unfused form of step_by -- the device does
// update_forces, the host does integrate_pre_force / retain / integrate_after_force on the synced vector.
template <class F>
struct IntegratorT {
    virtual ~IntegratorT() = default;
    virtual void init() {}
    virtual void integrate_pre_force(std::vector<PointParticleT<F>>& points, F dt) = 0;
    virtual void integrate_after_force(std::vector<PointParticleT<F>>& points, F dt) = 0;
};

// shared.rs:106-149 restated on the host (the same products in the same order: compile without FMA contraction and
// a strict-math run through step_by_with equals the device-integrated run bit for bit)
template <class F>
struct LeapFrogIntegratorT : IntegratorT<F> {
    void integrate_pre_force(std::vector<PointParticleT<F>>& points, F dt) override {
        for (auto& p : points)
            for (int k = 0; k < 3; ++k) p.position[k] += (p.velocity[k] * F(0.5)) * dt;          // :138
    }
    void integrate_after_force(std::vector<PointParticleT<F>>& points, F dt) override {
        for (auto& p : points)
            for (int k = 0; k < 3; ++k) {
                p.velocity[k] += p.acceleration[k] * dt;                                          // :144
                p.position[k] += (p.velocity[k] * F(0.5)) * dt;                                   // :146
            }
    }
};

template <class F>
class SimulationT {
public:
    using Particle = PointParticleT<F>;
    virtual ~SimulationT() { if (h_) nbody_destroy(h_); }
    SimulationT(const SimulationT&) = delete;
    SimulationT& operator=(const SimulationT&) = delete;

    void init() { check(nbody_init(h_)); }                                  // shared.rs:85
    void step() { push_settings(); check(nbody_steps(h_, 1)); dirty_ = true; }   // :86-88
    void steps(int k) { push_settings(); check(nbody_steps(h_, k)); dirty_ = true; }  // k x step(), no host sync
    void step_by(F dt) { push_settings(); check(abi::step_by(h_, dt)); dirty_ = true; }  // :89
    void update_forces() { push_settings(); check(nbody_update_forces(h_)); dirty_ = true; }  // :90
    void add_point(const Particle& p) { check(nbody_add_point(h_, &p)); dirty_ = true; }  // :91
    void remove_point(size_t index) { check(nbody_remove_point(h_, index)); dirty_ = true; }   // :92 (swap_remove)
    const std::vector<Particle>& get_points() const {                       // :93
        if (dirty_) {
            size_t n = 0;
            check(nbody_count(h_, &n));
            points_.resize(n);
            check(nbody_download(h_, points_.data(), n, sizeof(Particle), &n));
            points_.resize(n);
            dirty_ = false;
        }
        return points_;
    }
    // step_by with the integrator `I` of the caller's choice (the trait's generic parameter): brute_force.rs:84-90 /
    // barnes_hut.rs:265-271 step by step -- pre-force on the host, retain (Bounds::contains, shared.rs:210-212: inclusive
    // walls, NaN dropped, order kept), forces on the device, after-force on the host, elapsed += dt
    void step_by_with(IntegratorT<F>& integrator, F dt) {
        push_settings();
        std::vector<Particle> pts = get_points();
        integrator.integrate_pre_force(pts, dt);
        const F hw = bounds_.width * F(0.5);
        size_t kept = 0;
        for (size_t i = 0; i < pts.size(); ++i) {
            bool in = true;
            for (int k = 0; k < 3; ++k) {
                const F lo = bounds_.center[k] + (-hw), hi = bounds_.center[k] + hw;
                if (!(pts[i].position[k] >= lo) || !(pts[i].position[k] <= hi)) in = false;
            }
            if (in) pts[kept++] = pts[i];
        }
        pts.resize(kept);
        check(nbody_upload(h_, pts.data(), pts.size(), sizeof(Particle)));
        check(nbody_update_forces(h_));
        dirty_ = true;
        pts = get_points();
        integrator.integrate_after_force(pts, dt);
        check(nbody_upload(h_, pts.data(), pts.size(), sizeof(Particle)));
        points_ = std::move(pts);
        dirty_ = false;
        host_elapsed_ += dt;
    }
    F elapsed() const { F t = 0; check(abi::elapsed(h_, &t)); return t + host_elapsed_; }   // :94
    const SimulationSettingsT<F>& settings() const { return settings_; }    // :95
    SimulationSettingsT<F>& settings_mut() { settings_dirty_ = true; return settings_; }  // :96
    void sync() { check(nbody_sync(h_)); }
    NbodyStats stats() { NbodyStats s{}; check(nbody_stats(h_, &s)); return s; }
    // acceleration and potential of all bodies at n caller-chosen points (f64 triples); acc [n][3] / phi [n] may be null;
    // mode: NBODY_POTENTIAL_PAIRS, NBODY_POTENTIAL_TREE, or NBODY_POTENTIAL_TREE_QUADRUPOLE (f32 single-shard Barnes-Hut handles)
    void field_at(int mode, const double* xyz, size_t n, double* acc, double* phi, uint64_t counts[2] = nullptr) {
        push_settings();
        check(nbody_field_at(h_, mode, xyz, n, acc, phi, counts));
    }
    // the tidal tensor d acc_a / d x_b of all bodies at n caller-chosen points (f64 triples): tidal6 [n][6] = {xx, xy, xz, yy, yz, zz},
    // null only counts; mode: NBODY_POTENTIAL_PAIRS or NBODY_POTENTIAL_TREE (self-gravity only, monopole terms)
    void tidal_at(int mode, const double* xyz, size_t n, double* tidal6, uint64_t counts[2] = nullptr) {
        push_settings();
        check(nbody_tidal_at(h_, mode, xyz, n, tidal6, counts));
    }
    // order of the Barnes-Hut force walk's expansion (nbody_set_multipole): NBODY_MULTIPOLE_MONOPOLE, or NBODY_MULTIPOLE_QUADRUPOLE
    // on f32 fast-math single-shard Barnes-Hut handles; from the next force pass on
    void set_multipole(int order) { check(nbody_set_multipole(h_, order)); }
    int multipole() const { int order = 0; check(nbody_get_multipole(h_, &order)); return order; }
    // what step(), steps() and step_by() advance the bodies with (nbody_set_integrator): NBODY_INTEGRATOR_LEAPFROG, or
    // NBODY_INTEGRATOR_HERMITE4 on brute-force f64 handles of a one-rank world
    void set_integrator(int integrator) { check(nbody_set_integrator(h_, integrator)); }
    int integrator() const { int which = 0; check(nbody_get_integrator(h_, &which)); return which; }
    // block individual time steps of a Hermite handle (nbody_set_block_steps): eta > 0 and 1 <= max_level <= 20 switch them on,
    // (0, 0) off; step_by(dt) is then a macro step of 2^max_level ticks and steps() synchronises with the host
    void set_block_steps(double eta, int max_level) { check(nbody_set_block_steps(h_, eta, max_level)); }
    void block_steps(double* eta, int* max_level) const { check(nbody_get_block_steps(h_, eta, max_level)); }
    std::vector<int32_t> levels() {   // per body, in get_points() order; refused while the levels are invalid
        size_t n = 0;
        check(nbody_count(h_, &n));
        std::vector<int32_t> out(n);
        check(nbody_download_levels(h_, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    void block_step_counts(uint64_t out[2]) { check(nbody_block_step_counts(h_, out)); }   // {block steps, body updates}
    // tracers: massless particles in the bodies' field (nbody_tracers_*): PointParticle<f32,3> records whatever F is, the mass
    // ignored; f32 handles of a one-rank world (brute force and Barnes-Hut), every other handle throws NBODY_ERR_INVALID
    void set_tracers(const std::vector<PointParticleT<float>>& rec, size_t capacity = 0) {
        check(nbody_tracers_upload(h_, rec.data(), rec.size(), sizeof(PointParticleT<float>), capacity));
    }
    std::vector<PointParticleT<float>> get_tracers() {   // acc = the last tracer force pass, mass = 0
        size_t n = 0;
        check(nbody_tracers_count(h_, &n));
        std::vector<PointParticleT<float>> out(n);
        check(nbody_tracers_download(h_, out.data(), out.size(), sizeof(PointParticleT<float>), &n));
        out.resize(n);
        return out;
    }
    size_t n_tracers() { size_t n = 0; check(nbody_tracers_count(h_, &n)); return n; }
    void tracer_stats(uint64_t out[2]) { check(nbody_tracer_stats(h_, out)); }   // {directed interactions, opening tests}
    // a static external field acting on bodies and tracers (nbody_set_external_field): at most NBODY_EXTERNAL_MAX components,
    // an empty vector removes it; leapfrog handles of a one-rank world, every other handle throws NBODY_ERR_INVALID
    void set_external_field(const std::vector<NbodyExternalComponent>& comps) {
        check(nbody_set_external_field(h_, comps.data(), comps.size()));
    }
    std::vector<NbodyExternalComponent> external_field() const {
        std::vector<NbodyExternalComponent> out(NBODY_EXTERNAL_MAX);
        size_t n = 0;
        check(nbody_get_external_field(h_, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    // mesh gravity (nbody_set_mesh_gravity): while set, the self-gravity pass of every step and of update_forces is the mesh field
    // of pm_field with g := the handle's g, rounded once to the handle's dtype; clear_mesh_gravity switches it off.  Brute-force
    // leapfrog handles of a one-rank world, every other handle throws NBODY_ERR_INVALID.  mesh_gravity: false while it is off.
    // mesh_gravity_stats: {passes enqueued, the plan the last one used, 3-D transforms enqueued, allocations of the resident state}
    void set_mesh_gravity(const NbodyGridSpec& spec, const NbodyPmSpec& pm) { check(nbody_set_mesh_gravity(h_, &spec, &pm)); }
    void clear_mesh_gravity() { check(nbody_set_mesh_gravity(h_, nullptr, nullptr)); }
    bool mesh_gravity(NbodyGridSpec* spec, NbodyPmSpec* pm) const {
        int on = 0;
        check(nbody_get_mesh_gravity(h_, spec, pm, &on));
        return on != 0;
    }
    void mesh_gravity_stats(uint64_t out[4]) { check(nbody_mesh_gravity_stats(h_, out)); }
    std::vector<double> external_potentials() {   // phi_ext per body, in get_points() order, f64
        size_t n = 0;
        check(nbody_count(h_, &n));
        std::vector<double> out(n);
        check(nbody_external_potentials(h_, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    // sum m_i phi_ext(x_i): the conserved total is KE + PE + this (nbody_energy stays self-gravity only)
    double external_energy() { double v = 0; check(nbody_external_energy(h_, &v)); return v; }
    void external_at(const double* xyz, size_t n, double* acc, double* phi) { push_settings(); check(nbody_external_at(h_, xyz, n, acc, phi)); }
    // diagnostics of the state as a whole (nbody_moments, nbody_lagrangian_radii): f64 on either F, read-only, evaluated on the
    // device; handles of a one-rank world, every other handle throws NBODY_ERR_INVALID
    void moments(double out[10]) { check(nbody_moments(h_, out)); }   // {M, X[3] = sum m x, P[3], L[3] about the origin}
    // radii[k]: the distance from center (nullptr: the centre of mass) within which fractions[k] of the mass lies; returns the mass
    double lagrangian_radii(const double* center, const std::vector<double>& fractions, std::vector<double>& radii) {
        double mass = 0;
        radii.assign(fractions.size(), 0.0);
        check(nbody_lagrangian_radii(h_, center, fractions.data(), fractions.size(), radii.data(), &mass));
        return mass;
    }
    // binary census (nbody_partners, nbody_bound_pairs): f64 on either F, read-only, O(N^2) pair energies on the device; the
    // handles moments() takes.  partner[i] = the body of least two-body energy with i (-1: none), energy[i] = that energy
    void partners(std::vector<int32_t>& partner, std::vector<double>& energy) {
        size_t n = 0;
        push_settings();   // (g and g_soft enter the pair energy)
        check(nbody_partners(h_, nullptr, nullptr, 0, &n));
        partner.assign(n, -1);
        energy.assign(n, 0.0);
        check(nbody_partners(h_, partner.data(), energy.data(), n, &n));
        partner.resize(n);
        energy.resize(n);
    }
    // the mutual bound pairs in ascending i, i < j, with their orbital elements; returns the sum of their binding energies
    double bound_pairs(std::vector<NbodyBoundPair>& pairs) {
        size_t n = 0;
        double sum = 0;
        push_settings();
        check(nbody_partners(h_, nullptr, nullptr, 0, &n));   // (counts only: n bodies hold at most n / 2 pairs)
        pairs.assign(n / 2 + 1, NbodyBoundPair{});
        check(nbody_bound_pairs(h_, pairs.data(), pairs.size(), &n, &sum));
        pairs.resize(n);
        return sum;
    }
    // sticky mergers (nbody_nearest, nbody_contacts, nbody_merge_contacts): f64 unsoftened distances on either F, O(N^2) on the
    // device; the handles moments() takes.  nearest[i] = the body at the least squared distance from i (-1: none), dist2[i] = it
    void nearest(std::vector<int32_t>& nearest, std::vector<double>& dist2) {
        size_t n = 0;
        check(nbody_nearest(h_, nullptr, nullptr, 0, &n));
        nearest.assign(n, -1);
        dist2.assign(n, 0.0);
        check(nbody_nearest(h_, nearest.data(), dist2.data(), n, &n));
        nearest.resize(n);
        dist2.resize(n);
    }
    // the mutual nearest pairs closer than `radius` (strictly), in ascending i, i < j; read-only
    std::vector<NbodyContact> contacts(double radius) {
        size_t n = 0;
        check(nbody_nearest(h_, nullptr, nullptr, 0, &n));   // (counts only: n bodies hold at most n / 2 contacts)
        std::vector<NbodyContact> list(n / 2 + 1);
        check(nbody_contacts(h_, radius, list.data(), list.size(), &n));
        list.resize(n);
        return list;
    }
    // the same pairs merged: body i becomes the pair's centre of mass, body j is removed, everybody else keeps their order.
    // One call merges disjoint pairs: repeat while the list is not empty.
    std::vector<NbodyContact> merge_contacts(double radius) {
        size_t n = 0;
        check(nbody_nearest(h_, nullptr, nullptr, 0, &n));
        std::vector<NbodyContact> list(n / 2 + 1);
        check(nbody_merge_contacts(h_, radius, list.data(), list.size(), &n));
        list.resize(n);
        if (n) dirty_ = true;
        return list;
    }
    // friends-of-friends groups (nbody_fof_labels, nbody_fof_groups): bodies closer than the linking length b (strictly, f64
    // unsoftened distances on either F) are friends, a group is a connected component; read-only, the handles moments() takes.
    // labels[i] = the lowest index of i's group; returns the number of groups, singletons included
    size_t fof_labels(double b, std::vector<int32_t>& labels) {
        size_t n = 0, n_groups = 0;
        check(nbody_fof_labels(h_, b, nullptr, 0, &n, nullptr));   // (the bodies only)
        labels.assign(n, -1);
        check(nbody_fof_labels(h_, b, labels.data(), n, &n, &n_groups));
        labels.resize(n);
        return n_groups;
    }
    // the groups of at least min_members bodies in ascending `first`, and their bodies, group after group, each in ascending
    // index: group k's are members[offset .. offset + count)
    std::vector<NbodyGroup> fof_groups(double b, std::vector<int32_t>& members, int min_members = 2) {
        size_t n = 0, n_groups = 0, n_members = 0;
        check(nbody_fof_labels(h_, b, nullptr, 0, &n, nullptr));   // (the bodies only: an upper bound of both counts)
        std::vector<NbodyGroup> groups(n / size_t(min_members > 0 ? min_members : 1) + 1);
        members.assign(n + 1, -1);
        check(nbody_fof_groups(h_, b, min_members, groups.data(), groups.size(), &n_groups, members.data(), members.size(), &n_members));
        groups.resize(n_groups);
        members.resize(n_members);
        return groups;
    }
    // the self-bound subsets of those groups (nbody_fof_bound_groups): every member's energy inside its own group, the unbound
    // stripped at once, repeated until nobody is unbound or max_iterations passes have run; groups left with fewer than
    // min_members (>= 2) bodies are dropped.  members and energy (the e of the group's last pass) are parallel
    std::vector<NbodyBoundGroup> fof_bound_groups(double b, std::vector<int32_t>& members, std::vector<double>& energy, int min_members = 2,
                                                  int max_iterations = 32) {
        size_t n = 0, n_groups = 0, n_members = 0;
        check(nbody_fof_labels(h_, b, nullptr, 0, &n, nullptr));   // (the bodies only: an upper bound of both counts)
        std::vector<NbodyBoundGroup> groups(n / size_t(min_members > 0 ? min_members : 1) + 1);
        members.assign(n + 1, -1);
        energy.assign(n + 1, 0.0);
        check(nbody_fof_bound_groups(h_, b, min_members, max_iterations, groups.data(), groups.size(), &n_groups, members.data(),
                                     members.size(), &n_members, energy.data()));
        groups.resize(n_groups);
        members.resize(n_members);
        energy.resize(n_members);
        return groups;
    }
    // neighbours within a radius (nbody_neighbors_within, nbody_density, nbody_density_center): f64 unsoftened distances on
    // either F, strictly inside the radius; read-only, the handles moments() takes.  The neighbours of body i are
    // neighbor[offset[i] .. offset[i + 1]) in ascending index; offset has n + 1 entries
    void neighbors_within(double radius, std::vector<uint64_t>& offset, std::vector<int32_t>& neighbor) {
        size_t n = 0;
        uint64_t total = 0;
        check(nbody_neighbors_within(h_, radius, nullptr, 0, nullptr, 0, &n, &total));   // (counts only)
        offset.assign(n + 1, 0);
        neighbor.assign(size_t(total), -1);
        check(nbody_neighbors_within(h_, radius, offset.data(), n, total ? neighbor.data() : nullptr, size_t(total), &n, &total));
        offset.resize(n + 1);
        neighbor.resize(size_t(total));
    }
    // rho[i]: the density at body i from its neighbours within `radius` and itself (kernel: NBODY_KERNEL_TOP_HAT or
    // NBODY_KERNEL_CUBIC_SPLINE), count[i]: the number of terms
    void density(double radius, int kernel, std::vector<double>& rho, std::vector<int32_t>& count) {
        size_t n = 0;
        check(nbody_density(h_, radius, kernel, nullptr, nullptr, 0, &n));   // (the bodies)
        rho.assign(n, 0.0);
        count.assign(n, 0);
        check(nbody_density(h_, radius, kernel, rho.data(), count.data(), n, &n));
        rho.resize(n);
        count.resize(n);
    }
    // the density-weighted centre (what lagrangian_radii's `center` wants); returns the sum of the densities
    double density_center(double radius, int kernel, double center[3]) {
        double sum = 0;
        check(nbody_density_center(h_, radius, kernel, center, &sum));
        return sum;
    }
    // k nearest neighbours (nbody_knn, nbody_knn_density, nbody_knn_density_center): exact, f64 unsoftened distances on either F;
    // read-only, the handles moments() takes.  Row i of neighbor / dist2 (k entries each) holds the k bodies j != i first in
    // (r2 ascending, j ascending) and their r2, padded with -1 and +inf; radius_hint (0: none) never changes the result -- under
    // NBODY_SEARCH_CELLS the rows that find k bodies inside it are answered from the cells; stats = {those rows, the others}
    void knn(int k, double radius_hint, std::vector<int32_t>& neighbor, std::vector<double>& dist2, uint64_t stats[2] = nullptr) {
        size_t n = 0;
        check(nbody_knn(h_, k, radius_hint, nullptr, nullptr, 0, &n, nullptr));   // (counts only)
        neighbor.assign(n * size_t(k), -1);
        dist2.assign(n * size_t(k), 0.0);
        check(nbody_knn(h_, k, radius_hint, n ? neighbor.data() : nullptr, n ? dist2.data() : nullptr, n, &n, stats));
        neighbor.resize(n * size_t(k));
        dist2.resize(n * size_t(k));
    }
    // rho[i]: Casertano & Hut's density at body i from its k nearest neighbours (k >= 2), rk2[i]: the squared distance to the k-th
    void knn_density(int k, double radius_hint, std::vector<double>& rho, std::vector<double>& rk2) {
        size_t n = 0;
        check(nbody_knn_density(h_, k, radius_hint, nullptr, nullptr, 0, &n));   // (the bodies)
        rho.assign(n, 0.0);
        rk2.assign(n, 0.0);
        check(nbody_knn_density(h_, k, radius_hint, n ? rho.data() : nullptr, n ? rk2.data() : nullptr, n, &n));
        rho.resize(n);
        rk2.resize(n);
    }
    // the centre weighted with that density (what lagrangian_radii's `center` wants); returns the sum of the densities
    double knn_density_center(int k, double radius_hint, double center[3]) {
        double sum = 0;
        check(nbody_knn_density_center(h_, k, radius_hint, center, &sum));
        return sum;
    }
    // pair-separation counts (nbody_pair_counts, nbody_pair_counts_at): counts[b] = the pairs whose unsoftened f64 squared
    // separation r2 has edges[b]^2 <= r2 < edges[b + 1]^2 (edges: n_bins + 1 of them), outside = {the pairs below edges[0]^2,
    // everything else}; integers, read-only, the handles moments() takes.  pair_counts: every pair i < j of bodies, honours
    // set_pair_search; pair_counts_at: every (body, point) pair for xyz = m points {x, y, z}, always over all pairs
    void pair_counts(const std::vector<double>& edges, std::vector<uint64_t>& counts, uint64_t outside[2]) {
        counts.assign(edges.empty() ? 0 : edges.size() - 1, 0);
        check(nbody_pair_counts(h_, edges.data(), int(edges.size()) - 1, counts.data(), outside));
    }
    void pair_counts_at(const std::vector<double>& xyz, const std::vector<double>& edges, std::vector<uint64_t>& counts, uint64_t outside[2]) {
        counts.assign(edges.empty() ? 0 : edges.size() - 1, 0);
        check(nbody_pair_counts_at(h_, xyz.data(), xyz.size() / 3, edges.data(), int(edges.size()) - 1, counts.data(), outside));
    }
    // grid deposit (nbody_deposit): the bodies' quantity (spec.quantity: NBODY_DEPOSIT_MASS ...) assigned to the cells of
    // spec by NBODY_DEPOSIT_NGP / CIC / TSC in 64-bit fixed point -- the same state gives the same bits --; grid = [nx][ny][nz]
    // row-major, counts = {inside, partial, outside, skipped}; read-only, the handles moments() takes.  deposit_stats: {a call
    // reached the device, its plan, terms on the grid, 64-bit atomics sent to global memory} (nbody_deposit_stats).
    // host_deposit: the same arithmetic on the host for n points {x, y, z} and their q (nbody_host_deposit; no device)
    void deposit(const NbodyGridSpec& spec, std::vector<double>& grid, uint64_t counts[4]) {
        grid.assign(size_t(spec.dims[0] > 0 ? spec.dims[0] : 0) * size_t(spec.dims[1] > 0 ? spec.dims[1] : 0) *
                        size_t(spec.dims[2] > 0 ? spec.dims[2] : 0), 0.0);
        check(nbody_deposit(h_, &spec, grid.empty() ? nullptr : grid.data(), grid.size(), counts));
    }
    void deposit_stats(uint64_t out[4]) { check(nbody_deposit_stats(h_, out)); }
    static int host_deposit(const double* xyz, const double* q, size_t n, const NbodyGridSpec& spec, double* grid, size_t cap, uint64_t counts[4]) {
        return nbody_host_deposit(xyz, q, n, &spec, grid, cap, counts);
    }
    // grid sample (nbody_grid_sample, nbody_grid_sample_at): grid = [fields][nx][ny][nz] read back with spec's NBODY_DEPOSIT_NGP /
    // CIC / TSC weights (the transpose of deposit) at the bodies, in get_points() order, or at the n points xyz = {x, y, z}; op =
    // NBODY_SAMPLE_VALUE (out [n][fields]) or NBODY_SAMPLE_GRADIENT2 / 4 (+grad of one field by central differences, out [n][3]);
    // cls = each row's class, counts = {inside, partial, outside, skipped}; read-only, the handles deposit() takes.
    // grid_sample_stats: {a call reached the device, the plan it used, grid reads of the sample kernel, 0}.  host_grid_sample:
    // the same arithmetic on the host (nbody_host_grid_sample; no device)
    void grid_sample(const NbodyGridSpec& spec, const std::vector<double>& grid, int fields, int op, std::vector<double>& out,
                     std::vector<uint8_t>& cls, uint64_t counts[4]) {
        const size_t width = op == NBODY_SAMPLE_VALUE ? size_t(fields > 0 ? fields : 0) : 3;
        size_t n = 0;
        check(nbody_count(h_, &n));
        out.assign(n * width, 0.0);
        cls.assign(n, 0);
        check(nbody_grid_sample(h_, &spec, grid.data(), fields, op, out.data(), cls.data(), n, &n, counts));
        out.resize(n * width);
        cls.resize(n);
    }
    void grid_sample_at(const NbodyGridSpec& spec, const std::vector<double>& grid, int fields, int op, const std::vector<double>& xyz,
                        std::vector<double>& out, std::vector<uint8_t>& cls, uint64_t counts[4]) {
        const size_t n = xyz.size() / 3, width = op == NBODY_SAMPLE_VALUE ? size_t(fields > 0 ? fields : 0) : 3;
        out.assign(n * width, 0.0);
        cls.assign(n, 0);
        check(nbody_grid_sample_at(h_, &spec, grid.data(), fields, op, xyz.data(), n, out.data(), cls.data(), counts));
    }
    void grid_sample_stats(uint64_t out[4]) { check(nbody_grid_sample_stats(h_, out)); }
    static int host_grid_sample(const double* xyz, size_t n, const NbodyGridSpec& spec, const double* grid, int fields, int op, double* out,
                                uint8_t* cls, uint64_t counts[4]) {
        return nbody_host_grid_sample(xyz, n, &spec, grid, fields, op, out, cls, counts);
    }
    // grid Poisson (nbody_grid_poisson): phi [nx][ny][nz] at the cell centres from the mass per cell (deposit() with
    // NBODY_DEPOSIT_MASS; powers of two) by the library's own f64 FFT -- spec.periodic = 1: ps.green = NBODY_POISSON_SPECTRAL |
    // DIFF2, ps.deconvolve powers of the scheme's window; 0: zero padding, ps.soften.  The handle lends its stream and its memory
    // only.  grid_poisson_stats: {a call reached the device, the plan it used, butterfly launches, complex points transformed}.
    // host_grid_poisson, host_poisson_twiddles: the same arithmetic and its twiddle table on the host (no device)
    void grid_poisson(const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const std::vector<double>& mass, std::vector<double>& phi) {
        phi.assign(mass.size(), 0.0);
        check(nbody_grid_poisson(h_, &spec, &ps, mass.data(), phi.data(), phi.size()));
    }
    void grid_poisson_stats(uint64_t out[4]) { check(nbody_grid_poisson_stats(h_, out)); }
    static int host_grid_poisson(const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const double* mass, double* phi, size_t cap) {
        return nbody_host_grid_poisson(&spec, &ps, mass, phi, cap);
    }
    static int host_poisson_twiddles(int length, double* out) { return nbody_host_poisson_twiddles(length, out); }
    // particle-mesh field (nbody_pm_field, nbody_pm_field_at): deposit(NBODY_DEPOSIT_MASS), grid_poisson(pm.poisson) and
    // grid_sample(pm.gradient) composed on the device with the grid never leaving it: acc [n][3] = -grad phi, phi [n] (want_phi),
    // cls [n] = the gradient sample's classes, counts = the deposit's four then the sample's four; at the bodies, in get_points()
    // order, or at the n points xyz = {x, y, z}.  Read-only, the handles deposit() takes; the same bytes as host_pm_field
    // (nbody_host_pm_field; no device).  pm_field_stats: {a call reached the device, the plan it used, grid reads of the gather,
    // radix sorts enqueued}
    void pm_field(const NbodyGridSpec& spec, const NbodyPmSpec& pm, std::vector<double>& acc, std::vector<double>& phi, std::vector<uint8_t>& cls,
                  uint64_t counts[8], bool want_phi = true) {
        size_t n = 0;
        check(nbody_count(h_, &n));
        acc.assign(n * 3, 0.0);
        phi.assign(want_phi ? n : 0, 0.0);
        cls.assign(n, 0);
        check(nbody_pm_field(h_, &spec, &pm, acc.data(), want_phi ? phi.data() : nullptr, cls.data(), n, &n, counts));
        acc.resize(n * 3);
        phi.resize(want_phi ? n : 0);
        cls.resize(n);
    }
    void pm_field_at(const NbodyGridSpec& spec, const NbodyPmSpec& pm, const std::vector<double>& xyz, std::vector<double>& acc,
                     std::vector<double>& phi, std::vector<uint8_t>& cls, uint64_t counts[8], bool want_phi = true) {
        const size_t n = xyz.size() / 3;
        acc.assign(n * 3, 0.0);
        phi.assign(want_phi ? n : 0, 0.0);
        cls.assign(n, 0);
        check(nbody_pm_field_at(h_, &spec, &pm, xyz.data(), n, acc.data(), want_phi ? phi.data() : nullptr, cls.data(), counts));
    }
    void pm_field_stats(uint64_t out[4]) { check(nbody_pm_field_stats(h_, out)); }
    static int host_pm_field(const double* body_xyz, const double* body_m, size_t n_bodies, const NbodyGridSpec& spec, const NbodyPmSpec& pm,
                             const double* xyz, size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t counts[8]) {
        return nbody_host_pm_field(body_xyz, body_m, n_bodies, &spec, &pm, xyz, n_points, acc, phi, cls, counts);
    }
    // P3M field (nbody_p3m_field, nbody_p3m_field_at): pm_field on a periodic grid with the Gaussian split of scale p.r_split in its
    // Green stage, plus the minimum-image pair sum of the bodies closer than p.r_cut (p.terms picks both parts or one); shapes, cls
    // and counts as pm_field's.  Read-only; the same bits as host_p3m_field (nbody_host_p3m_field; no device).  host_p3m_table:
    // the split factors {F, P} [4097][2].  p3m_field_stats: {a call reached the device, the plan it used, partners looked at,
    // terms with r2 < R2}
    void p3m_field(const NbodyGridSpec& spec, const NbodyP3mSpec& p, std::vector<double>& acc, std::vector<double>& phi, std::vector<uint8_t>& cls,
                   uint64_t counts[8], bool want_phi = true) {
        size_t n = 0;
        check(nbody_count(h_, &n));
        acc.assign(n * 3, 0.0);
        phi.assign(want_phi ? n : 0, 0.0);
        cls.assign(n, 0);
        check(nbody_p3m_field(h_, &spec, &p, acc.data(), want_phi ? phi.data() : nullptr, cls.data(), n, &n, counts));
        acc.resize(n * 3);
        phi.resize(want_phi ? n : 0);
        cls.resize(n);
    }
    void p3m_field_at(const NbodyGridSpec& spec, const NbodyP3mSpec& p, const std::vector<double>& xyz, std::vector<double>& acc,
                      std::vector<double>& phi, std::vector<uint8_t>& cls, uint64_t counts[8], bool want_phi = true) {
        const size_t n = xyz.size() / 3;
        acc.assign(n * 3, 0.0);
        phi.assign(want_phi ? n : 0, 0.0);
        cls.assign(n, 0);
        check(nbody_p3m_field_at(h_, &spec, &p, xyz.data(), n, acc.data(), want_phi ? phi.data() : nullptr, cls.data(), counts));
    }
    void p3m_field_stats(uint64_t out[4]) { check(nbody_p3m_field_stats(h_, out)); }
    static int host_p3m_field(const double* body_xyz, const double* body_m, size_t n_bodies, const NbodyGridSpec& spec, const NbodyP3mSpec& p,
                              const double* xyz, size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t counts[8]) {
        return nbody_host_p3m_field(body_xyz, body_m, n_bodies, &spec, &p, xyz, n_points, acc, phi, cls, counts);
    }
    static int host_p3m_table(double r_split, double r_cut, double* out) { return nbody_host_p3m_table(r_split, r_cut, out); }
    // how fof_labels, fof_groups, contacts, merge_contacts, neighbors_within, density, density_center and pair_counts find their pairs
    // (nbody_set_pair_search): NBODY_SEARCH_ALL_PAIRS, or
    // NBODY_SEARCH_CELLS -- the bodies sorted by the cell of a uniform grid; it changes no result.  pair_search_stats: {1 if the
    // last of those calls ran the cell search, bodies gridded, occupied cells, candidate pairs} (nbody_pair_search_stats)
    void set_pair_search(int mode) { check(nbody_set_pair_search(h_, mode)); }
    int pair_search() const { int mode = 0; check(nbody_get_pair_search(h_, &mode)); return mode; }
    void pair_search_stats(uint64_t out[4]) { check(nbody_pair_search_stats(h_, out)); }
    // the grid that search would draw for n points {x, y, z} (nbody_host_cell_grid; host only)
    static int host_cell_grid(const double* xyz, size_t n, double length, double lo[3], double* side, uint64_t* key, int* usable) {
        return nbody_host_cell_grid(xyz, n, length, lo, side, key, usable);
    }
    NbodyHandle* handle() { return h_; }

protected:
    SimulationT(int method, const std::vector<Particle>& points, const BoundsT<F>& bounds, int math_mode,
                size_t capacity, int host_threads, int tree_build = NBODY_TREE_AUTO,
                int leaf_mode = NBODY_LEAF_REFERENCE) : bounds_(bounds) {
        NbodyConfig cfg{};
        cfg.struct_size = sizeof(cfg);
        cfg.method = method;
        cfg.math_mode = math_mode;
        cfg.leaf_mode = leaf_mode;
        cfg.device = -1;
        cfg.rank = 0;
        cfg.world_size = 1;
        cfg.host_threads = host_threads;
        cfg.capacity = capacity ? capacity : (points.empty() ? 1 : points.size());
        cfg.tree_build = tree_build;
        cfg.dtype = abi::dtype_of<F>();
        int rc = nbody_create(&cfg, &h_);
        if (rc) throw Error(rc, nbody_last_error(nullptr));
        check(abi::set_bounds(h_, bounds.center.data(), bounds.width));
        check(nbody_upload(h_, points.data(), points.size(), sizeof(Particle)));
    }
    explicit SimulationT(NbodyHandle* cloned, const SimulationT& src)
        : h_(cloned), settings_(src.settings_), bounds_(src.bounds_) {}
    NbodyHandle* clone_handle() const {                                     // `Clone` supertrait
        NbodyHandle* c = nullptr;
        int rc = nbody_clone(h_, &c);
        if (rc) throw Error(rc, nbody_last_error(nullptr));
        return c;
    }
    void check(int rc) const { if (rc) throw Error(rc, nbody_last_error(h_)); }
    void push_settings() {
        if (!settings_dirty_) return;
        check(abi::set_settings(h_, settings_.g, settings_.g_soft, settings_.dt, settings_.theta2));
        settings_dirty_ = false;
    }

    NbodyHandle* h_ = nullptr;
    SimulationSettingsT<F> settings_{};
    BoundsT<F> bounds_{};
    bool settings_dirty_ = true;
    F host_elapsed_ = F(0);   // advanced by step_by_with (the device's clock only sees its own steps)
    mutable bool dirty_ = true;
    mutable std::vector<Particle> points_;
};
using Simulation = SimulationT<float>;

// Simulation::new(points, LeapFrogIntegrator::new(), bounds) for the two solvers of src/manual
template <class F>
class BruteForceSimulationT : public SimulationT<F> {
public:
    BruteForceSimulationT(const std::vector<PointParticleT<F>>& points, const BoundsT<F>& bounds,
                          int math_mode = NBODY_MATH_FAST, size_t capacity = 0)
        : SimulationT<F>(NBODY_BRUTE_FORCE, points, bounds, math_mode, capacity, 0) {}
    std::unique_ptr<BruteForceSimulationT> clone() const {
        return std::unique_ptr<BruteForceSimulationT>(new BruteForceSimulationT(this->clone_handle(), *this));
    }
private:
    BruteForceSimulationT(NbodyHandle* h, const SimulationT<F>& src) : SimulationT<F>(h, src) {}
};
using BruteForceSimulation = BruteForceSimulationT<float>;

template <class F>
class BarnesHutSimulationT : public SimulationT<F> {
public:
    BarnesHutSimulationT(const std::vector<PointParticleT<F>>& points, const BoundsT<F>& bounds,
                         int math_mode = NBODY_MATH_FAST, size_t capacity = 0, int host_threads = 0,
                         int tree_build = NBODY_TREE_AUTO, int leaf_mode = NBODY_LEAF_REFERENCE)
        : SimulationT<F>(NBODY_BARNES_HUT, points, bounds, math_mode, capacity, host_threads, tree_build, leaf_mode) {}
    std::unique_ptr<BarnesHutSimulationT> clone() const {
        return std::unique_ptr<BarnesHutSimulationT>(new BarnesHutSimulationT(this->clone_handle(), *this));
    }
private:
    BarnesHutSimulationT(NbodyHandle* h, const SimulationT<F>& src) : SimulationT<F>(h, src) {}
};
using BarnesHutSimulation = BarnesHutSimulationT<float>;

}  // namespace nbody
