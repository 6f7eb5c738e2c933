// nbody_mesh.cpp -- mesh gravity (include/nbody_hip.h, "mesh gravity"): what a handle keeps on the device between passes -- the
// one particle-mesh scratch with the Poisson tables in it and, on an isolated grid, the transformed kernel -- and the pass
// itself: nbody_pm.cpp's stages enqueued against that scratch, then kernels_mesh.hip's gather into the shard's acc rows.
// Nothing here is waited for unless the resident state has to be made or regrown.
#include "nbody_mesh.h"

#include "nbody_pm.h"
#include "nbody_poisson.h"   // kHeldTables, kHeldKernel
#include "kernels.h"         // launch_kick_drift

#include <cstring>
#include <memory>

namespace nbody { namespace mesh {

// The resident state.  `block` is the handle's registry's; everything else is the host's description of it.
struct Resident {
    void* block = nullptr;
    size_t cap_bodies = 0, cap_rows = 0;   // what the layout holds: body rows of the deposit, rows of the gather (bodies or tracers)
    NbodyGridSpec spec{};                  // the spec and the PM spec (g apart) the tables and the layout were made for
    NbodyPmSpec pm{};
    int layout_key[5] = {-1, -1, -1, -1, -1};   // the knobs the carving depends on
    std::unique_ptr<pm::Call> call;        // the grid, the shape and the tables (their source on the host outlives every copy)
    pm::Scratch w;
    bool kernel_made = false;              // w.poi.k holds the transformed kernel of spec (isolated)
};

const char* refusal(const NbodyHandle* h) {
    if (h->cfg.method != NBODY_BRUTE_FORCE) return "NBODY_BARNES_HUT handles take no mesh gravity (their unsynchronised-step accounting is out of scope)";
    if (h->let || h->cfg.shard_mode != NBODY_SHARD_INDEX) return "NBODY_SHARD_SPATIAL handles take no mesh gravity (out of scope)";
    if (h->cfg.world_size != 1) return "handles of a multi-rank world take no mesh gravity (out of scope)";
    return nullptr;
}

void set(NbodyHandle* h, const NbodyGridSpec& spec, const NbodyPmSpec& pm) {
    MeshGravity& m = h->mesh;
    std::memcpy(&m.spec, &spec, sizeof(spec));
    std::memcpy(&m.pm, &pm, sizeof(pm));
    m.on = true;   // (a resident state made for another spec is remade by the next pass)
}

int clear(NbodyHandle* h) {
    MeshGravity& m = h->mesh;
    m.on = false;
    if (!m.res) return NBODY_OK;
    const hipError_t e = hipStreamSynchronize(h->stream);   // (a pass that is still enqueued reads the block)
    h->mem.free_dev(m.res->block);
    delete m.res;
    m.res = nullptr;
    HIP_TRY(h, e);
    return NBODY_OK;
}

void destroy(NbodyHandle* h) {
    delete h->mesh.res;   // (its block is the registry's)
    h->mesh.res = nullptr;
}

namespace {

NbodyPmSpec without_g(NbodyPmSpec pm) {
    pm.poisson.g = 0.0;   // (not read by a pass: the handle's g is)
    return pm;
}

// The resident state for n_bodies body rows and n_tracers tracer rows under the current knobs: made at the first pass, remade
// when the spec, the carving or a bound outgrows it -- before the pass enqueues anything -- and left alone otherwise.
int ensure(NbodyHandle* h, size_t n_bodies, size_t n_tracers, const Plan& mp) {
    MeshGravity& m = h->mesh;
    if (!m.res) m.res = new Resident();
    Resident& r = *m.res;
    const NbodyPmSpec pm = without_g(m.pm);
    const bool same_spec = r.call && std::memcmp(&r.spec, &m.spec, sizeof(m.spec)) == 0 && std::memcmp(&r.pm, &pm, sizeof(pm)) == 0;
    if (!same_spec) {
        r.call.reset(new pm::Call(m.spec, pm, true));
        std::memcpy(&r.spec, &m.spec, sizeof(m.spec));
        std::memcpy(&r.pm, &pm, sizeof(pm));
    }
    pm::Call& c = *r.call;
    c.plans = pm::make_plans(c.op, deposit::cells_of(c.g), true);
    if (mp.kick_fuse) c.plans.grad.pregrad = 0;   // (k_mesh_kick forms the differences on the fly)
    const pm::Plans& p = c.plans;
    const int key[5] = {p.dep.sort, p.shared ? 1 : 0, p.grad.sort, p.grad.pregrad, p.pm.gather};
    const size_t rows = std::max(n_bodies, n_tracers);
    if (same_spec && r.block && std::equal(key, key + 5, r.layout_key) && n_bodies <= r.cap_bodies && rows <= r.cap_rows) return NBODY_OK;
    // a new block: whatever is enqueued against the old one is waited for first
    if (r.block) HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->mem.free_dev(r.block);
    r.kernel_made = false;
    const size_t cap_bodies = std::max<size_t>(std::max(n_bodies, r.cap_bodies), 1), cap_rows = std::max(std::max(rows, r.cap_rows), cap_bodies);
    r.cap_bodies = r.cap_rows = 0;
    HIP_TRY(h, hipError_t(h->mem.dev(r.block, pm::scratch_bytes(cap_bodies, cap_rows, c.g, c.shape, c.deconvolve, c.op, p))));
    m.allocations += 1;
    r.w = pm::scratch_layout(r.block, cap_bodies, cap_rows, c.g, c.shape, c.deconvolve, c.op, p);
    r.cap_bodies = cap_bodies;
    r.cap_rows = cap_rows;
    std::copy(key, key + 5, r.layout_key);
    // the Poisson tables, once per block
    const hipError_t e = poisson::upload_tables(h, c.tables, r.w.poi);
    HIP_TRY(h, e);
    return NBODY_OK;
}

// the gather of one vector of rows (the bodies, or the tracers) against the resident grid: w.smp.xyz holds their positions;
// ordered: w.smp.rows + n holds their home-cell order already
template <class F>
void rows_pass(NbodyHandle* h, const Resident& r, const Plan& mp, const ShardT<F>& sh, size_t n, bool ordered, const F* kick_dt, Enqueued& st,
               pm::Tally& tally) {
    const hipStream_t s = h->stream;
    const pm::Call& c = *r.call;
    const pm::Scratch& w = r.w;
    if (!st.ok()) return;
    if (mp.kick_fuse) {
        int rc = 0;
        const int* rows = sample::ordered_rows(s, sh.own_count(), int(n), c.g, w.smp, c.plans.grad.sort != 0, ordered, &rc, &tally.sorts);
        st.prim(rc);
        if (st.ok()) launch_kick<F>(s, sh, sh.own_count(), int(n), c.g, c.op, rows, w, kick_dt);
        return;
    }
    // the cross-check: nbody_pm_field's own rows in f64, rounded, and the leapfrog's own kick
    pm::enqueue_rows(h, c, sh.own_count(), n, false, ordered, w, st, tally);
    if (!st.ok()) return;
    launch_round<F>(s, sh, sh.own_count(), int(n), w.smp.out);
    if (kick_dt) nbody::launch_kick_drift<F>(s, sh, int(n), *kick_dt);
}

}  // namespace

template <class F>
int pass(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double g, const F* kick_dt, const float* tracer_kick_dt) {
    MeshGravity& m = h->mesh;
    const size_t n_tracers = h->tr.n_host;
    if (!n_upper && !n_tracers) return NBODY_OK;
    const Plan mp = make_plan();
    int rc = ensure(h, n_upper, n_tracers, mp);
    if (rc) return rc;
    Resident& r = *m.res;
    pm::Call& c = *r.call;
    NbodyPmSpec pm = r.pm;
    pm.poisson.g = g;
    c.tables.c = poisson::green_constant(g, m.spec.spacing);
    const pm::Scratch& w = r.w;
    const hipStream_t s = h->stream;
    Enqueued st;   // (nothing is waited for: the resident state outlives the pass, and result() is asked, not finish())
    pm::Tally tally;
    sample::launch_stage<F>(s, sh, int(n_upper), w.smp);
    const bool shared = c.plans.shared && n_upper > 0;   // one order for the deposit and the gather, as in nbody_pm_field
    const int* order = pm::enqueue_shared_order(h, c, sh.own_count(), n_upper, shared, w, st, tally);
    const bool keep = mp.keep_kernel && r.kernel_made && !c.shape.periodic;
    pm::enqueue_grid<F>(h, sh, n_upper, m.spec, pm, c, w, order, st, tally, poisson::kHeldTables | (keep ? poisson::kHeldKernel : 0));
    m.transforms += tally.transforms;
    if (st.ok()) {
        r.kernel_made = !c.shape.periodic;
        if (n_upper) rows_pass<F>(h, r, mp, sh, n_upper, shared, kick_dt, st, tally);
    }
    if (st.ok() && n_tracers) {   // the tracers, at their own positions against the same grid
        const Shard& t = h->tr.sh;
        sample::launch_stage<float>(s, t, int(n_tracers), w.smp);
        rows_pass<float>(h, r, mp, t, n_tracers, false, tracer_kick_dt, st, tally);
    }
    st.last();
    if (const int rc = st.result(h, "mesh gravity")) return rc;
    m.passes += 1;
    m.last_plan = uint64_t(mp.code()) | uint64_t(c.plans.pm.gather | (c.plans.shared ? 2 : 0)) << 2;
    return NBODY_OK;
}

template int pass<float>(NbodyHandle*, const ShardT<float>&, size_t, double, const float*, const float*);
template int pass<double>(NbodyHandle*, const ShardT<double>&, size_t, double, const double*, const float*);

}}  // namespace nbody::mesh
