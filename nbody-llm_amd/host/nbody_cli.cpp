// nbody_cli.cpp -- the reference's headless driver (src/main.rs:31-129) over the HIP engine.
// Keeps the argv contract `-t <threads> -n <points>` that perf_benchmark.py:107-112 drives, the
// disc initial conditions (main.rs:52-89), the hard-coded settings dt = 3e-2, g_soft = 0.02,
// theta2 = 1.0 (main.rs:103-105), the 1000-step loop and the two output lines
//     Elapsed: <duration>
//     Performance: <x> steps/second
// (main.rs:124-128).  Extra flags select what the reference needs a source edit for; --dtype f64 runs the
// reference's own precision (PointParticle<f64,3>, main.rs:52-105); --integrator host steps through the trait's generic
// `Integrator` parameter (shared.rs:99-104) with a leapfrog on the host instead of the device's fused one, --integrator
// hermite runs the device's fourth-order Hermite step (--method bf --dtype f64 only; leapfrog = device, the default); --dump FILE
// writes the final PointParticle records; --multipole 2 adds the cells' quadrupole terms to the Barnes-Hut force walk;
// --tracers M scatters M massless tracers in the workload's disc or sphere (the IC generator with seed + 1) and reports their
// interactions per second on a line of its own; --external KIND:p0:p1[...][:cx:cy:cz] (repeatable; plummer:M:b, hernquist:M:a,
// mn:M:a:b, log:v0:rc:qy:qz) adds a component of a static external field and reports the external energy before and after;
// --diagnostics prints M, |P|, |L| and the 10 / 50 / 90 % Lagrangian radii about the centre of mass before and after the run,
// and the binary census of the final state (nbody_bound_pairs) on a line of its own; --pairs prints that line alone;
// --merge RADIUS[:EVERY] runs nbody_merge_contacts after every EVERY-th step (default 1: sticky spheres of that merge distance)
// and prints how many bodies were absorbed, in how many calls, on a line of its own; --fof B[:MIN] prints the friends-of-friends
// groups of the final state for the linking length B (nbody_fof_groups): how many have at least MIN members (default 2), the
// members and the mass of the largest, and the fraction of bodies in no listed group; --fof-bound ITER (with --fof) prints one
// more line after it: the self-bound subsets of those groups after at most ITER unbinding passes (nbody_fof_bound_groups, at
// least max(MIN, 2) members): how many groups, their members, how many FoF groups dissolved, and the members, kinetic and
// potential energy of the largest; --pair-search cells lets --merge and
// --fof find their pairs over the cells of a uniform grid (nbody_set_pair_search: the same results) and prints what the last
// such call gridded on a line of its own; --density R[:tophat|spline] (default spline) prints the density centre of the final
// state (nbody_density_center), the largest density and its body (nbody_density) and the half-mass Lagrangian radius about
// that centre, on a line of its own, and honours --pair-search; --pair-counts LO:HI:BINS[:log|lin] (default log, which needs
// LO > 0) prints the binned pair-separation counts of the final state (nbody_pair_counts), one line per bin with its two edges
// and its count, then the `outside` line, and honours --pair-search; --knn K[:HINT] prints, for the final state, the median and
// the largest distance to a body's K-th nearest neighbour (nbody_knn; among the bodies that have K), how many rows the cells and
// the all-pairs pass answered (HINT and --pair-search cells: the same numbers otherwise) and, for K >= 2, the Casertano-Hut
// density centre (nbody_knn_density_center), on a line of its own.  The BINS + 1 edges of --pair-counts are formed here in f64:
//     edges[0] = LO,  edges[BINS] = HI,  and for 0 < b < BINS
//     lin: edges[b] = LO + (HI - LO) * (double(b) / double(BINS))      log: edges[b] = LO * pow(HI / LO, double(b) / double(BINS))
// and printed with 17 significant digits, which name each double exactly.  --deposit ngp|cic|tsc:N:HALF prints the mass of
// the final state assigned to the N^3 cells of the cube [-HALF, HALF)^3 (nbody_deposit; spacing = (2 HALF) / N in f64): one
// line with the four counts, one with the sum over the cells (in cell order) and the heaviest cell.  --sample value|grad2|grad4
// (with --deposit only) reads that mass grid back at the bodies of the final state with the same spec (nbody_grid_sample): one
// line with the four counts, then the first eight bodies' outputs with 17 significant digits.  --poisson isolated|spectral|diff2
// (with --deposit only, N a power of two) solves Poisson's equation on that mass grid (nbody_grid_poisson; the periodic modes
// deposit with wrapped indices): one line with the mode and the grid, one with the sum of phi and its lowest cell.  --pm
// isolated|spectral|diff2:grad2|grad4 (with --deposit only, N a power of two) is the three of them in one call (nbody_pm_field):
// one line with the mode, the gradient and the eight counts, then the first eight bodies' acc and phi with 17 significant digits.
// --p3m spectral|diff2:grad2|grad4 (with --deposit only) is the P3M field at the bodies (nbody_p3m_field) on that grid taken as
// periodic, r_split = 1.25 spacing, r_cut = 4.5 r_split: one line with the counts and the pair counts, then the first bodies.
// --mesh isolated|spectral|diff2:grad2|grad4 (with --deposit only, N a power of two) steps under mesh gravity on that grid
// (nbody_set_mesh_gravity): one line with the mode, the gradient, the plan and the words of nbody_mesh_gravity_stats, then the
// first eight bodies' position and acceleration.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "simulation.hpp"

static void usage() {
    std::fprintf(stderr,
                 "usage: nbody_cli [-t threads] [-n points] [--method bh|bf] [--ic disc|plummer] [--steps K]\n"
                 "                 [--math fast|strict] [--tree auto|host|device] [--leaf reference|direct]\n"
                 "                 [--dtype f32|f64] [--dt x] [--g-soft x] [--theta2 x]\n"
                 "                 [--width w] [--seed s] [--integrator device|leapfrog|host|hermite] [--dump file] [--multipole 1|2]\n"
                 "                 [--block-steps ETA:LEVELS]   (with --integrator hermite: block individual time steps)\n"
                 "                 [--tracers M]   (massless tracers in the same disc or sphere; --dtype f32)\n"
                 "                 [--external plummer:M:b[:cx:cy:cz] | hernquist:M:a[...] | mn:M:a:b[...] | log:v0:rc:qy:qz[...]]   (repeatable)\n"
                 "                 [--diagnostics]   (M, |P|, |L| and the 10/50/90 %% Lagrangian radii before and after the run, and --pairs)\n"
                 "                 [--pairs]   (the mutual bound pairs of the final state: count, binding energy, the hardest pair)\n"
                 "                 [--merge RADIUS[:EVERY]]   (after every EVERY-th step, merge the mutual nearest pairs closer than RADIUS)\n"
                 "                 [--fof B[:MIN]]   (the friends-of-friends groups of the final state: linking length B, at least MIN members, default 2)\n"
                 "                 [--fof-bound ITER]   (with --fof: the self-bound subsets of those groups after at most ITER unbinding passes)\n"
                 "                 [--density R[:tophat|spline]]   (the density centre of the final state, the largest density, r50 about that centre)\n"
                 "                 [--pair-counts LO:HI:BINS[:log|lin]]   (the pairs of the final state per bin of separation; log needs LO > 0)\n"
                 "                 [--knn K[:HINT]]   (every body's K nearest neighbours, 1 <= K <= 32: the median and largest K-th distance, the Casertano-Hut centre)\n"
                 "                 [--deposit ngp|cic|tsc:N:HALF]   (the mass of the final state on the N^3 cells of [-HALF, HALF)^3)\n"
                 "                 [--sample value|grad2|grad4]   (with --deposit: that grid read back at the bodies, its value or its gradient)\n"
                 "                 [--pm isolated|spectral|diff2:grad2|grad4]   (with --deposit, N a power of two: the mesh acceleration and potential at the bodies in one call)\n"
                 "                 [--p3m spectral|diff2:grad2|grad4]   (with --deposit, N a power of two with N / 8 >= 4: the P3M field at the bodies on that grid taken as periodic, r_split = 1.25 spacing, r_cut = 4.5 r_split)\n"
                 "                 [--mesh isolated|spectral|diff2:grad2|grad4]   (with --deposit, N a power of two: the steps run under mesh gravity on that grid, no pair kernel)\n"
                 "                 [--poisson isolated|spectral|diff2]   (with --deposit, N a power of two: the potential of that mass grid, zero-padded or periodic)\n"
                 "                 [--pair-search all|cells]  (how --merge, --fof, --density, --pair-counts and --knn (with a HINT) find their pairs: all pairs, or the cells of a uniform grid)\n");
}

// KIND:p...[:cx:cy:cz] -> a component; false if the text is not one
static bool parse_external(const char* arg, NbodyExternalComponent* out) {
    static const struct { const char* name; int kind; int n_par; } kinds[] = {
        {"plummer", NBODY_EXT_PLUMMER, 2}, {"hernquist", NBODY_EXT_HERNQUIST, 2}, {"mn", NBODY_EXT_MIYAMOTO_NAGAI, 3}, {"log", NBODY_EXT_LOGARITHMIC, 4}};
    const char* colon = std::strchr(arg, ':');
    if (!colon) return false;
    const std::string name(arg, colon);
    for (const auto& k : kinds) {
        if (name != k.name) continue;
        std::vector<double> v;
        const char* at = colon;
        while (*at == ':') {
            char* end = nullptr;
            v.push_back(std::strtod(at + 1, &end));
            if (end == at + 1) return false;
            at = end;
        }
        if (*at || (v.size() != size_t(k.n_par) && v.size() != size_t(k.n_par) + 3)) return false;
        *out = NbodyExternalComponent{};
        out->kind = k.kind;
        for (int i = 0; i < k.n_par; ++i) out->p[i] = v[size_t(i)];
        if (v.size() > size_t(k.n_par)) for (int i = 0; i < 3; ++i) out->center[i] = v[size_t(k.n_par + i)];
        return true;
    }
    return false;
}

// one line of --diagnostics: nbody_moments and nbody_lagrangian_radii about the centre of mass
template <class Sim>
static void print_diagnostics(Sim& sim, const char* when) {
    double m[10];
    sim.moments(m);
    std::vector<double> radii;
    const double mass = sim.lagrangian_radii(nullptr, {0.1, 0.5, 0.9}, radii);
    std::printf("Diagnostics %s: M %.9e  |P| %.9e  |L| %.9e  r10 %.9e  r50 %.9e  r90 %.9e  mass in radii %.9e\n", when, m[0],
                std::sqrt(m[4] * m[4] + m[5] * m[5] + m[6] * m[6]), std::sqrt(m[7] * m[7] + m[8] * m[8] + m[9] * m[9]), radii[0], radii[1],
                radii[2], mass);
}

// the line of --pairs: nbody_bound_pairs; the hardest pair is the one of least binding energy (the first of equals)
template <class Sim>
static void print_pairs(Sim& sim) {
    std::vector<NbodyBoundPair> pairs;
    const double sum = sim.bound_pairs(pairs);
    size_t hard = 0;
    for (size_t k = 1; k < pairs.size(); ++k) if (pairs[k].binding < pairs[hard].binding) hard = k;
    const double nan = std::nan("");
    std::printf("Bound pairs: %zu binding %.9e hardest a=%.9e e=%.9e\n", pairs.size(), sum, pairs.empty() ? nan : pairs[hard].semi_major,
                pairs.empty() ? nan : pairs[hard].eccentricity);
}

// the line of --fof: nbody_fof_groups; the largest group is the one of most members (the first of equals)
template <class Sim>
static void print_fof(Sim& sim, double b, int min_members) {
    std::vector<int32_t> members;
    const std::vector<NbodyGroup> groups = sim.fof_groups(b, members, min_members);
    size_t big = 0;
    for (size_t k = 1; k < groups.size(); ++k) if (groups[k].count > groups[big].count) big = k;
    const size_t n = sim.get_points().size();
    std::printf("FoF groups: %zu largest %d mass %.9e ungrouped %.6f\n", groups.size(), groups.empty() ? 0 : groups[big].count,
                groups.empty() ? 0.0 : groups[big].mass, n ? double(n - members.size()) / double(n) : 0.0);
}

// the line of --fof-bound: nbody_fof_bound_groups on the groups of at least max(min_members, 2) bodies; the largest bound group
// is the one of most bound members (the first of equals)
template <class Sim>
static void print_fof_bound(Sim& sim, double b, int min_members, int max_iterations) {
    const int least = min_members > 2 ? min_members : 2;
    std::vector<int32_t> members;
    std::vector<double> energy;
    const size_t fof_groups = sim.fof_groups(b, members, least).size();
    const std::vector<NbodyBoundGroup> groups = sim.fof_bound_groups(b, members, energy, least, max_iterations);
    size_t big = 0;
    for (size_t k = 1; k < groups.size(); ++k) if (groups[k].count > groups[big].count) big = k;
    std::printf("FoF bound groups: %zu members %zu dissolved %zu largest %d kinetic %.9e potential %.9e\n", groups.size(), members.size(),
                fof_groups - groups.size(), groups.empty() ? 0 : groups[big].count, groups.empty() ? 0.0 : groups[big].kinetic,
                groups.empty() ? 0.0 : groups[big].potential);
}

// the line of --density: nbody_density_center, nbody_density (the densest body: the first of equals) and the half-mass
// Lagrangian radius about the density centre
template <class Sim>
static void print_density(Sim& sim, double radius, int kernel) {
    double center[3];
    const double rho_sum = sim.density_center(radius, kernel, center);
    std::vector<double> rho, radii;
    std::vector<int32_t> count;
    sim.density(radius, kernel, rho, count);
    size_t top = 0;
    for (size_t k = 1; k < rho.size(); ++k) if (rho[k] > rho[top]) top = k;
    sim.lagrangian_radii(center, {0.5}, radii);
    std::printf("Density: center %.17e %.17e %.17e rho_sum %.17e max %.17e body %ld terms %d r50 %.17e\n", center[0], center[1], center[2], rho_sum,
                rho.empty() ? std::nan("") : rho[top], rho.empty() ? -1L : long(top), rho.empty() ? 0 : int(count[top]), radii[0]);
}

// the line of --knn: nbody_knn (the K-th distances of the complete rows, sorted; the median is the upper one of an even number)
// and, for K >= 2, nbody_knn_density_center
template <class Sim>
static void print_knn(Sim& sim, int k, double hint) {
    std::vector<int32_t> neighbor;
    std::vector<double> dist2, rk;
    uint64_t stats[2] = {0, 0};
    sim.knn(k, hint, neighbor, dist2, stats);
    for (size_t i = 0; i * size_t(k) < dist2.size(); ++i)
        if (neighbor[i * size_t(k) + size_t(k - 1)] >= 0) rk.push_back(std::sqrt(dist2[i * size_t(k) + size_t(k - 1)]));
    std::sort(rk.begin(), rk.end());
    const double nan = std::nan("");
    std::printf("kNN: k %d rk median %.17e max %.17e cells %llu all-pairs %llu", k, rk.empty() ? nan : rk[rk.size() / 2],
                rk.empty() ? nan : rk.back(), (unsigned long long)stats[0], (unsigned long long)stats[1]);
    if (k >= 2) {
        double center[3];
        sim.knn_density_center(k, hint, center);
        std::printf(" center %.17e %.17e %.17e", center[0], center[1], center[2]);
    }
    std::printf("\n");
}

// the edges of --pair-counts (the formula stands at the top of this file)
static std::vector<double> pair_count_edges(double lo, double hi, int bins, bool log_bins) {
    std::vector<double> edges(size_t(bins) + 1);
    for (int b = 0; b <= bins; ++b) {
        const double f = double(b) / double(bins);
        edges[size_t(b)] = b == 0 ? lo : b == bins ? hi : log_bins ? lo * std::pow(hi / lo, f) : lo + (hi - lo) * f;
    }
    return edges;
}

// the lines of --pair-counts: nbody_pair_counts over `edges`
template <class Sim>
static void print_pair_counts(Sim& sim, const std::vector<double>& edges) {
    std::vector<uint64_t> counts;
    uint64_t outside[2] = {0, 0};
    sim.pair_counts(edges, counts, outside);
    for (size_t b = 0; b < counts.size(); ++b)
        std::printf("Pair count: bin %zu %.17e %.17e %llu\n", b, edges[b], edges[b + 1], (unsigned long long)counts[b]);
    std::printf("Pair counts outside: below %llu beyond %llu\n", (unsigned long long)outside[0], (unsigned long long)outside[1]);
}

// the lines of --deposit: nbody_deposit of the mass over spec
template <class Sim>
static void print_deposit(Sim& sim, const NbodyGridSpec& spec) {
    std::vector<double> grid;
    uint64_t counts[4] = {0, 0, 0, 0};
    sim.deposit(spec, grid, counts);
    double sum = 0.0;
    size_t top = 0;
    for (size_t c = 0; c < grid.size(); ++c) {
        sum += grid[c];
        if (grid[c] > grid[top]) top = c;
    }
    const size_t ny = size_t(spec.dims[1]), nz = size_t(spec.dims[2]);
    std::printf("Deposit: scheme %d dims %d %d %d spacing %.17e inside %llu partial %llu outside %llu skipped %llu\n", spec.scheme, spec.dims[0],
                spec.dims[1], spec.dims[2], spec.spacing, (unsigned long long)counts[0], (unsigned long long)counts[1],
                (unsigned long long)counts[2], (unsigned long long)counts[3]);
    std::printf("Deposit sum %.17e max %.17e at %zu %zu %zu\n", sum, grid.empty() ? 0.0 : grid[top], top / (ny * nz), top / nz % ny, top % nz);
}

// the lines of --sample: the mass grid of --deposit read back at the bodies with the same spec (nbody_grid_sample)
template <class Sim>
static void print_sample(Sim& sim, const NbodyGridSpec& spec, int op) {
    std::vector<double> grid, out;
    std::vector<uint8_t> cls;
    uint64_t counts[4] = {0, 0, 0, 0};
    sim.deposit(spec, grid, counts);
    sim.grid_sample(spec, grid, 1, op, out, cls, counts);
    const size_t width = op == NBODY_SAMPLE_VALUE ? 1 : 3;
    std::printf("Sample: op %d bodies %zu inside %llu partial %llu outside %llu skipped %llu\n", op, cls.size(), (unsigned long long)counts[0],
                (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3]);
    for (size_t i = 0; i < cls.size() && i < 8; ++i) {
        std::printf("Sample body %zu class %d", i, int(cls[i]));
        for (size_t k = 0; k < width; ++k) std::printf(" %.17e", out[i * width + k]);
        std::printf("\n");
    }
}

// the lines of --poisson: the mass grid of --deposit (wrapped for the periodic modes) solved for the potential (nbody_grid_poisson)
template <class Sim>
static void print_poisson(Sim& sim, NbodyGridSpec spec, int mode, double g) {
    std::vector<double> mass, phi;
    uint64_t counts[4] = {0, 0, 0, 0};
    spec.periodic = mode > 0;
    sim.deposit(spec, mass, counts);
    NbodyPoissonSpec ps{};
    ps.g = g;
    ps.green = mode == 2 ? NBODY_POISSON_DIFF2 : NBODY_POISSON_SPECTRAL;
    sim.grid_poisson(spec, ps, mass, phi);
    double sum = 0.0;
    size_t low = 0;
    for (size_t c = 0; c < phi.size(); ++c) {
        sum += phi[c];
        if (phi[c] < phi[low]) low = c;
    }
    const size_t ny = size_t(spec.dims[1]), nz = size_t(spec.dims[2]);
    std::printf("Poisson: %s g %.17e dims %d %d %d spacing %.17e\n", mode == 0 ? "isolated" : mode == 1 ? "periodic spectral" : "periodic diff2", g,
                spec.dims[0], spec.dims[1], spec.dims[2], spec.spacing);
    std::printf("Poisson sum %.17e min %.17e at %zu %zu %zu\n", sum, phi.empty() ? 0.0 : phi[low], low / (ny * nz), low / nz % ny, low % nz);
}

// the lines of --pm: the mesh field at the bodies in one call (nbody_pm_field): the boundary condition of --poisson, the gradient
// of --sample; then the first eight bodies' acc and phi with 17 significant digits
template <class Sim>
static void print_pm(Sim& sim, NbodyGridSpec spec, int mode, int gradient, double g) {
    std::vector<double> acc, phi;
    std::vector<uint8_t> cls;
    uint64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    spec.periodic = mode > 0;
    NbodyPmSpec pm{};
    pm.poisson.g = g;
    pm.poisson.green = mode == 2 ? NBODY_POISSON_DIFF2 : NBODY_POISSON_SPECTRAL;
    pm.gradient = gradient;
    sim.pm_field(spec, pm, acc, phi, cls, counts);
    std::printf("PM: %s gradient %d g %.17e bodies %zu deposited %llu %llu %llu %llu sampled %llu %llu %llu %llu\n",
                mode == 0 ? "isolated" : mode == 1 ? "periodic spectral" : "periodic diff2", gradient, g, cls.size(), (unsigned long long)counts[0],
                (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3], (unsigned long long)counts[4],
                (unsigned long long)counts[5], (unsigned long long)counts[6], (unsigned long long)counts[7]);
    for (size_t i = 0; i < cls.size() && i < 8; ++i)
        std::printf("PM body %zu class %d %.17e %.17e %.17e %.17e\n", i, int(cls[i]), acc[3 * i], acc[3 * i + 1], acc[3 * i + 2], phi[i]);
}

// the lines of --p3m: the P3M field at the bodies in one call (nbody_p3m_field) on the periodic grid of --deposit with r_split =
// 1.25 spacing, r_cut = 4.5 r_split and no softening; then the first eight bodies' acc and phi with 17 significant digits
template <class Sim>
static void print_p3m(Sim& sim, NbodyGridSpec spec, int mode, int gradient, double g) {
    std::vector<double> acc, phi;
    std::vector<uint8_t> cls;
    uint64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st[4] = {0, 0, 0, 0};
    spec.periodic = 1;
    NbodyP3mSpec p{};
    p.pm.poisson.g = g;
    p.pm.poisson.green = mode == 2 ? NBODY_POISSON_DIFF2 : NBODY_POISSON_SPECTRAL;
    p.pm.gradient = gradient;
    p.r_split = 1.25 * spec.spacing;
    p.r_cut = 4.5 * p.r_split;
    p.terms = NBODY_P3M_BOTH;
    sim.p3m_field(spec, p, acc, phi, cls, counts);
    sim.p3m_field_stats(st);
    std::printf("P3M: %s gradient %d g %.17e r_split %.17e r_cut %.17e bodies %zu deposited %llu %llu %llu %llu sampled %llu %llu %llu %llu partners %llu terms %llu\n",
                mode == 2 ? "periodic diff2" : "periodic spectral", gradient, g, p.r_split, p.r_cut, cls.size(), (unsigned long long)counts[0],
                (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3], (unsigned long long)counts[4],
                (unsigned long long)counts[5], (unsigned long long)counts[6], (unsigned long long)counts[7], (unsigned long long)st[2],
                (unsigned long long)st[3]);
    for (size_t i = 0; i < cls.size() && i < 8; ++i)
        std::printf("P3M body %zu class %d %.17e %.17e %.17e %.17e\n", i, int(cls[i]), acc[3 * i], acc[3 * i + 1], acc[3 * i + 2], phi[i]);
}

// --mesh: the grid of --deposit and the mode as the (spec, PM spec) pair of nbody_set_mesh_gravity (pm.poisson.g is not read by a pass)
static NbodyPmSpec mesh_specs(NbodyGridSpec* spec, int mode, int gradient) {
    spec->periodic = mode > 0;
    NbodyPmSpec pm{};
    pm.poisson.g = 1.0;
    pm.poisson.green = mode == 2 ? NBODY_POISSON_DIFF2 : NBODY_POISSON_SPECTRAL;
    pm.gradient = gradient;
    return pm;
}

// the lines of --mesh: the plan and the words of nbody_mesh_gravity_stats, and the first bodies of the final state
template <class Sim>
static void print_mesh(Sim& sim, int mode, int gradient) {
    uint64_t ms[4] = {0, 0, 0, 0};
    sim.mesh_gravity_stats(ms);
    std::printf("MESH: %s gradient %d plan %llu passes %llu transforms %llu allocations %llu\n", mode == 0 ? "isolated" : mode == 1 ? "spectral" : "diff2",
                gradient, (unsigned long long)ms[1], (unsigned long long)ms[0], (unsigned long long)ms[2], (unsigned long long)ms[3]);
    const auto& pts = sim.get_points();
    for (size_t i = 0; i < pts.size() && i < 8; ++i)
        std::printf("MESH body %zu %.17e %.17e %.17e %.17e %.17e %.17e\n", i, double(pts[i].position[0]), double(pts[i].position[1]),
                    double(pts[i].position[2]), double(pts[i].acceleration[0]), double(pts[i].acceleration[1]), double(pts[i].acceleration[2]));
}

template <class F>
static int run(const std::string& method, const std::string& ic, const std::string& math, const std::string& tree,
               const std::string& leaf, size_t threads, size_t num_points, size_t steps, double dt, double g_soft, double theta2,
               double width, unsigned long long seed, const std::string& integrator, const std::string& dump, int multipole,
               double block_eta, int block_levels, size_t n_tracers, const std::vector<NbodyExternalComponent>& external,
               bool diagnostics, bool pairs, double merge_radius, size_t merge_every, double fof_b, int fof_min, int fof_bound, int pair_search,
               double density_radius, int density_kernel, const std::vector<double>& pair_edges, int knn_k, double knn_hint,
               const NbodyGridSpec* deposit_spec, int sample_op, int poisson_mode, int pm_mode, int pm_gradient, int mesh_mode,
               int mesh_gradient, int p3m_mode, int p3m_gradient) {
    using P = nbody::PointParticleT<F>;
    const bool wide = sizeof(F) == 8;
    std::vector<P> points;
    if (ic == "disc") {
        points.resize(num_points + 1);  // the star + n disc bodies
        if ((wide ? nbody_ic_disc_f64 : nbody_ic_disc)(points.data(), num_points, sizeof(P), seed)) return 1;
    } else {
        points.resize(num_points);
        if ((wide ? nbody_ic_plummer_f64 : nbody_ic_plummer)(points.data(), num_points, sizeof(P), seed)) return 1;
    }
    const int math_mode = math == "strict" ? NBODY_MATH_STRICT : NBODY_MATH_FAST;
    try {
        std::unique_ptr<nbody::SimulationT<F>> sim;
        nbody::BoundsT<F> bounds{{F(0), F(0), F(0)}, F(width)};
        if (method == "bf") sim.reset(new nbody::BruteForceSimulationT<F>(points, bounds, math_mode));
        else sim.reset(new nbody::BarnesHutSimulationT<F>(points, bounds, math_mode, 0, int(threads),
                                                         tree == "device" ? NBODY_TREE_DEVICE : tree == "host" ? NBODY_TREE_HOST : NBODY_TREE_AUTO,
                                                         leaf == "direct" ? NBODY_LEAF_DIRECT : NBODY_LEAF_REFERENCE));
        sim->settings_mut().dt = F(dt);
        sim->settings_mut().g_soft = F(g_soft);
        sim->settings_mut().theta2 = F(theta2);
        if (multipole != NBODY_MULTIPOLE_MONOPOLE) sim->set_multipole(multipole);   // (refused where it does not apply: nbody_hip.h)
        if (integrator == "hermite") sim->set_integrator(NBODY_INTEGRATOR_HERMITE4);
        if (pair_search != NBODY_SEARCH_ALL_PAIRS) sim->set_pair_search(pair_search);
        if (block_levels > 0) sim->set_block_steps(block_eta, block_levels);   // every --dt is then a macro step of 2^LEVELS ticks
        if (n_tracers) {   // the same generator with the next seed: tracers where the bodies are (the disc's star left out)
            std::vector<nbody::PointParticleT<float>> tr(n_tracers + 1);
            if (ic == "disc") { if (nbody_ic_disc(tr.data(), n_tracers, sizeof(tr[0]), seed + 1)) return 1; tr.erase(tr.begin()); }
            else { tr.resize(n_tracers); if (nbody_ic_plummer(tr.data(), n_tracers, sizeof(tr[0]), seed + 1)) return 1; }
            sim->set_tracers(tr);
        }
        if (!external.empty()) sim->set_external_field(external);   // (refused where it does not apply: nbody_hip.h)
        if (deposit_spec && mesh_mode >= 0) {   // (refused where it does not apply: nbody_hip.h)
            NbodyGridSpec spec = *deposit_spec;
            const NbodyPmSpec pm = mesh_specs(&spec, mesh_mode, mesh_gradient);
            sim->set_mesh_gravity(spec, pm);
        }
        std::printf("Running simulation without rendering...\n");  // main.rs:111
        sim->init();
        const double ext_before = external.empty() ? 0.0 : sim->external_energy();
        if (diagnostics) print_diagnostics(*sim, "before");
        size_t merged = 0, merge_calls = 0;
        const auto merge_after = [&](size_t i) {   // --merge: one call after step i + 1 when it is an EVERY-th one
            if (!(merge_radius > 0.0) || (i + 1) % merge_every) return;
            merged += sim->merge_contacts(merge_radius).size();
            merge_calls += 1;
        };
        auto start = std::chrono::steady_clock::now();
        if (integrator == "host") {   // the trait's generic Integrator, on the host (simulation.hpp step_by_with)
            nbody::LeapFrogIntegratorT<F> leapfrog;
            leapfrog.init();
            for (size_t i = 0; i < steps; ++i) { sim->step_by_with(leapfrog, F(dt)); merge_after(i); }
        } else {
            for (size_t i = 0; i < steps; ++i) { sim->step(); merge_after(i); }
        }
        sim->sync();
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        std::printf("Elapsed: %.6fs\n", secs);
        std::printf("Performance: %.2f steps/second\n", double(steps) / secs);
        NbodyStats st = sim->stats();
        std::printf("Bodies left: %zu  interactions/second: %.4e\n", sim->get_points().size(), double(st.interactions) / secs);
        if (n_tracers) {
            uint64_t ts[2] = {0, 0};
            sim->tracer_stats(ts);
            std::printf("Tracers left: %zu  tracer interactions/second: %.4e\n", sim->n_tracers(), double(ts[0]) / secs);
        }
        if (!external.empty()) std::printf("External energy: %.9e -> %.9e\n", ext_before, sim->external_energy());
        if (diagnostics) print_diagnostics(*sim, "after");
        if (diagnostics || pairs) print_pairs(*sim);
        if (merge_radius > 0.0) std::printf("Merged: %zu bodies in %zu calls\n", merged, merge_calls);
        if (fof_b > 0.0) print_fof(*sim, fof_b, fof_min);
        if (fof_b > 0.0 && fof_bound > 0) print_fof_bound(*sim, fof_b, fof_min, fof_bound);
        if (density_radius > 0.0) print_density(*sim, density_radius, density_kernel);
        if (!pair_edges.empty()) print_pair_counts(*sim, pair_edges);
        if (knn_k > 0) print_knn(*sim, knn_k, knn_hint);
        if (deposit_spec) print_deposit(*sim, *deposit_spec);
        if (deposit_spec && sample_op >= 0) print_sample(*sim, *deposit_spec, sample_op);
        if (deposit_spec && poisson_mode >= 0) print_poisson(*sim, *deposit_spec, poisson_mode, double(sim->settings_mut().g));
        if (deposit_spec && pm_mode >= 0) print_pm(*sim, *deposit_spec, pm_mode, pm_gradient, double(sim->settings_mut().g));
        if (deposit_spec && p3m_mode >= 0) print_p3m(*sim, *deposit_spec, p3m_mode, p3m_gradient, double(sim->settings_mut().g));
        if (deposit_spec && mesh_mode >= 0) print_mesh(*sim, mesh_mode, mesh_gradient);
        if (pair_search == NBODY_SEARCH_CELLS) {
            uint64_t ps[4] = {0, 0, 0, 0};
            sim->pair_search_stats(ps);
            std::printf("Pair search: cells %llu gridded %llu occupied %llu candidates %llu\n", (unsigned long long)ps[0], (unsigned long long)ps[1],
                        (unsigned long long)ps[2], (unsigned long long)ps[3]);
        }
        if (block_levels > 0) {
            uint64_t counts[2] = {0, 0};
            sim->block_step_counts(counts);
            std::printf("Block steps: %llu  body updates: %llu\n", (unsigned long long)counts[0], (unsigned long long)counts[1]);
        }
        if (!dump.empty()) {
            std::FILE* f = std::fopen(dump.c_str(), "wb");
            if (!f) { std::fprintf(stderr, "cannot write %s\n", dump.c_str()); return 1; }
            std::fwrite(sim->get_points().data(), sizeof(P), sim->get_points().size(), f);
            std::fclose(f);
        }
    } catch (const nbody::Error& e) {
        std::fprintf(stderr, "nbody error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    size_t threads = 0, num_points = 10000, steps = 1000;  // main.rs:33-38, :116
    std::string method = "bh", ic = "disc", math = "fast", tree = "auto", leaf = "reference", dtype = "f32", integrator = "device", dump;
    double dt = 3e-2, g_soft = 0.02, theta2 = 1.0, width = 10.0;  // main.rs:59,103-105
    unsigned long long seed = 20250523ull;
    int multipole = NBODY_MULTIPOLE_MONOPOLE;
    bool width_set = false;
    double block_eta = 0.0;
    int block_levels = 0;
    bool block_set = false;
    size_t n_tracers = 0;
    std::vector<NbodyExternalComponent> external;
    bool diagnostics = false, pairs = false;
    double merge_radius = 0.0;
    size_t merge_every = 1;
    double fof_b = 0.0;
    int pair_search = NBODY_SEARCH_ALL_PAIRS;
    int fof_min = 2, fof_bound = 0;
    double density_radius = 0.0;
    int density_kernel = NBODY_KERNEL_CUBIC_SPLINE;
    std::vector<double> pair_edges;
    int knn_k = 0;
    NbodyGridSpec deposit_spec{};
    bool deposit = false;
    int sample_op = -1;
    int poisson_mode = -1;   // 0 isolated, 1 periodic spectral, 2 periodic diff2
    int pm_mode = -1, pm_gradient = NBODY_SAMPLE_GRADIENT2;   // --pm: the same three modes, and the gradient
    int mesh_mode = -1, mesh_gradient = NBODY_SAMPLE_GRADIENT2;   // --mesh: the same again, as the step's self-gravity
    int p3m_mode = -1, p3m_gradient = NBODY_SAMPLE_GRADIENT2;     // --p3m: the two periodic modes, and the gradient
    double knn_hint = 0.0;
    for (int i = 1; i < argc; ++i) {
        auto next = [&]() -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        if (!std::strcmp(argv[i], "-t") || !std::strcmp(argv[i], "--threads")) threads = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "-n") || !std::strcmp(argv[i], "--num-points")) num_points = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--method")) method = next();
        else if (!std::strcmp(argv[i], "--ic")) ic = next();
        else if (!std::strcmp(argv[i], "--math")) math = next();
        else if (!std::strcmp(argv[i], "--tree")) tree = next();
        else if (!std::strcmp(argv[i], "--leaf")) leaf = next();
        else if (!std::strcmp(argv[i], "--dtype")) dtype = next();
        else if (!std::strcmp(argv[i], "--steps")) steps = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--dt")) dt = std::strtod(next(), nullptr);
        else if (!std::strcmp(argv[i], "--g-soft")) g_soft = std::strtod(next(), nullptr);
        else if (!std::strcmp(argv[i], "--theta2")) theta2 = std::strtod(next(), nullptr);
        else if (!std::strcmp(argv[i], "--width")) { width = std::strtod(next(), nullptr); width_set = true; }
        else if (!std::strcmp(argv[i], "--seed")) seed = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--integrator")) integrator = next();
        else if (!std::strcmp(argv[i], "--dump")) dump = next();
        else if (!std::strcmp(argv[i], "--multipole")) multipole = std::atoi(next());
        else if (!std::strcmp(argv[i], "--diagnostics")) diagnostics = true;
        else if (!std::strcmp(argv[i], "--pairs")) pairs = true;
        else if (!std::strcmp(argv[i], "--merge")) {
            char* end = nullptr;
            const char* arg = next();
            merge_radius = std::strtod(arg, &end);
            if (end == arg || !(merge_radius > 0.0) || !std::isfinite(merge_radius) || (*end && *end != ':')) { usage(); return 2; }
            if (*end == ':') {
                const long long every = std::atoll(end + 1);
                if (every < 1) { usage(); return 2; }
                merge_every = size_t(every);
            }
        }
        else if (!std::strcmp(argv[i], "--pair-search")) {
            const std::string mode = next();
            if (mode == "cells") pair_search = NBODY_SEARCH_CELLS;
            else if (mode == "all") pair_search = NBODY_SEARCH_ALL_PAIRS;
            else { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--fof")) {
            char* end = nullptr;
            const char* arg = next();
            fof_b = std::strtod(arg, &end);
            if (end == arg || !(fof_b > 0.0) || !std::isfinite(fof_b) || (*end && *end != ':')) { usage(); return 2; }
            if (*end == ':') {
                fof_min = std::atoi(end + 1);
                if (fof_min < 1) { usage(); return 2; }
            }
        }
        else if (!std::strcmp(argv[i], "--fof-bound")) {
            fof_bound = std::atoi(next());
            if (fof_bound < 1 || fof_bound > 1024) { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--pair-counts")) {
            char* end = nullptr;
            const char* arg = next();
            const double lo = std::strtod(arg, &end);
            if (end == arg || *end != ':') { usage(); return 2; }
            arg = end + 1;
            const double hi = std::strtod(arg, &end);
            if (end == arg || *end != ':') { usage(); return 2; }
            arg = end + 1;
            const long bins = std::strtol(arg, &end, 10);
            if (end == arg || (*end && *end != ':')) { usage(); return 2; }
            bool log_bins = true;
            if (*end == ':') {
                const std::string kind = end + 1;
                if (kind == "lin") log_bins = false;
                else if (kind != "log") { usage(); return 2; }
            }
            if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo >= 0.0) || !(hi > lo) || bins < 1 || bins > NBODY_PAIR_COUNT_MAX_BINS ||
                (log_bins && !(lo > 0.0))) { usage(); return 2; }
            pair_edges = pair_count_edges(lo, hi, int(bins), log_bins);
        }
        else if (!std::strcmp(argv[i], "--knn")) {
            char* end = nullptr;
            const char* arg = next();
            const long k = std::strtol(arg, &end, 10);
            if (end == arg || k < 1 || k > NBODY_KNN_MAX_K || (*end && *end != ':')) { usage(); return 2; }
            knn_k = int(k);
            if (*end == ':') {
                arg = end + 1;
                knn_hint = std::strtod(arg, &end);
                if (end == arg || *end || !(knn_hint > 0.0) || !std::isfinite(knn_hint)) { usage(); return 2; }
            }
        }
        else if (!std::strcmp(argv[i], "--deposit")) {
            const std::string arg = next();
            const size_t c1 = arg.find(':'), c2 = c1 == std::string::npos ? c1 : arg.find(':', c1 + 1);
            if (c2 == std::string::npos) { usage(); return 2; }
            const std::string scheme = arg.substr(0, c1);
            char* end = nullptr;
            const long cells = std::strtol(arg.c_str() + c1 + 1, &end, 10);
            if (end != arg.c_str() + c2) { usage(); return 2; }
            const double half = std::strtod(arg.c_str() + c2 + 1, &end);
            if (*end || !std::isfinite(half) || !(half > 0.0) || cells < 1 || cells > 512) { usage(); return 2; }
            if (scheme == "ngp") deposit_spec.scheme = NBODY_DEPOSIT_NGP;
            else if (scheme == "cic") deposit_spec.scheme = NBODY_DEPOSIT_CIC;
            else if (scheme == "tsc") deposit_spec.scheme = NBODY_DEPOSIT_TSC;
            else { usage(); return 2; }
            for (int c = 0; c < 3; ++c) { deposit_spec.origin[c] = -half; deposit_spec.dims[c] = int32_t(cells); }
            deposit_spec.spacing = (2.0 * half) / double(cells);
            deposit_spec.quantity = NBODY_DEPOSIT_MASS;
            deposit_spec.project_axis = -1;
            deposit = true;
        }
        else if (!std::strcmp(argv[i], "--sample")) {
            const std::string arg = next();
            if (arg == "value") sample_op = NBODY_SAMPLE_VALUE;
            else if (arg == "grad2") sample_op = NBODY_SAMPLE_GRADIENT2;
            else if (arg == "grad4") sample_op = NBODY_SAMPLE_GRADIENT4;
            else { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--poisson")) {
            const std::string arg = next();
            if (arg == "isolated") poisson_mode = 0;
            else if (arg == "spectral") poisson_mode = 1;
            else if (arg == "diff2") poisson_mode = 2;
            else { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--pm")) {
            const std::string arg = next();
            const size_t c = arg.find(':');
            if (c == std::string::npos) { usage(); return 2; }
            const std::string mode = arg.substr(0, c), grad = arg.substr(c + 1);
            if (mode == "isolated") pm_mode = 0;
            else if (mode == "spectral") pm_mode = 1;
            else if (mode == "diff2") pm_mode = 2;
            else { usage(); return 2; }
            if (grad == "grad2") pm_gradient = NBODY_SAMPLE_GRADIENT2;
            else if (grad == "grad4") pm_gradient = NBODY_SAMPLE_GRADIENT4;
            else { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--p3m")) {
            const std::string arg = next();
            const size_t c = arg.find(':');
            if (c == std::string::npos) { usage(); return 2; }
            const std::string mode = arg.substr(0, c), grad = arg.substr(c + 1);
            if (mode == "spectral") p3m_mode = 1;
            else if (mode == "diff2") p3m_mode = 2;
            else { usage(); return 2; }
            if (grad == "grad2") p3m_gradient = NBODY_SAMPLE_GRADIENT2;
            else if (grad == "grad4") p3m_gradient = NBODY_SAMPLE_GRADIENT4;
            else { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--mesh")) {
            const std::string arg = next();
            const size_t c = arg.find(':');
            if (c == std::string::npos) { usage(); return 2; }
            const std::string mode = arg.substr(0, c), grad = arg.substr(c + 1);
            if (mode == "isolated") mesh_mode = 0;
            else if (mode == "spectral") mesh_mode = 1;
            else if (mode == "diff2") mesh_mode = 2;
            else { usage(); return 2; }
            if (grad == "grad2") mesh_gradient = NBODY_SAMPLE_GRADIENT2;
            else if (grad == "grad4") mesh_gradient = NBODY_SAMPLE_GRADIENT4;
            else { usage(); return 2; }
        }
        else if (!std::strcmp(argv[i], "--density")) {
            char* end = nullptr;
            const char* arg = next();
            density_radius = std::strtod(arg, &end);
            if (end == arg || !(density_radius > 0.0) || !std::isfinite(density_radius) || (*end && *end != ':')) { usage(); return 2; }
            if (*end == ':') {
                const std::string kind = end + 1;
                if (kind == "tophat") density_kernel = NBODY_KERNEL_TOP_HAT;
                else if (kind == "spline") density_kernel = NBODY_KERNEL_CUBIC_SPLINE;
                else { usage(); return 2; }
            }
        }
        else if (!std::strcmp(argv[i], "--tracers")) n_tracers = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--external")) {
            NbodyExternalComponent c;
            if (!parse_external(next(), &c)) { usage(); return 2; }
            external.push_back(c);
        }
        else if (!std::strcmp(argv[i], "--block-steps")) {
            char* end = nullptr;
            const char* arg = next();
            block_eta = std::strtod(arg, &end);
            if (end == arg || *end != ':' || !(block_eta > 0.0)) { usage(); return 2; }
            block_levels = std::atoi(end + 1);
            if (block_levels < 1 || block_levels > 20) { usage(); return 2; }
            block_set = true;
        }
        else { usage(); return 2; }
    }
    if (integrator != "device" && integrator != "leapfrog" && integrator != "host" && integrator != "hermite") { usage(); return 2; }
    if (integrator == "hermite" && (dtype != "f64" || method != "bf")) {
        std::fprintf(stderr, "--integrator hermite needs --dtype f64 and --method bf\n");
        return 2;
    }
    if (block_set && integrator != "hermite") {
        std::fprintf(stderr, "--block-steps needs --integrator hermite\n");
        return 2;
    }
    if (!external.empty() && integrator == "hermite") {
        std::fprintf(stderr, "--external needs the leapfrog (the Hermite step would need the field's jerk)\n");
        return 2;
    }
    if (fof_bound && !(fof_b > 0.0)) {
        std::fprintf(stderr, "--fof-bound needs --fof\n");
        return 2;
    }
    if (sample_op >= 0 && !deposit) {
        std::fprintf(stderr, "--sample needs --deposit\n");
        return 2;
    }
    if (poisson_mode >= 0 && !deposit) {
        std::fprintf(stderr, "--poisson needs --deposit\n");
        return 2;
    }
    if (pm_mode >= 0 && !deposit) {
        std::fprintf(stderr, "--pm needs --deposit\n");
        return 2;
    }
    if (p3m_mode >= 0 && !deposit) {
        std::fprintf(stderr, "--p3m needs --deposit\n");
        return 2;
    }
    if (mesh_mode >= 0 && !deposit) {
        std::fprintf(stderr, "--mesh needs --deposit\n");
        return 2;
    }
    if (ic == "plummer" && !width_set) width = 64.0;
    if (dtype == "f64") return run<double>(method, ic, math, tree, leaf, threads, num_points, steps, dt, g_soft, theta2, width, seed, integrator, dump, multipole, block_eta, block_levels, n_tracers, external, diagnostics, pairs, merge_radius, merge_every, fof_b, fof_min, fof_bound, pair_search, density_radius, density_kernel, pair_edges, knn_k, knn_hint, deposit ? &deposit_spec : nullptr, sample_op, poisson_mode, pm_mode, pm_gradient, mesh_mode, mesh_gradient, p3m_mode, p3m_gradient);
    return run<float>(method, ic, math, tree, leaf, threads, num_points, steps, dt, g_soft, theta2, width, seed, integrator, dump, multipole, block_eta, block_levels, n_tracers, external, diagnostics, pairs, merge_radius, merge_every, fof_b, fof_min, fof_bound, pair_search, density_radius, density_kernel, pair_edges, knn_k, knn_hint, deposit ? &deposit_spec : nullptr, sample_op, poisson_mode, pm_mode, pm_gradient, mesh_mode, mesh_gradient, p3m_mode, p3m_gradient);
}
