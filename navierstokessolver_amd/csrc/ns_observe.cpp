// ns_observe.cpp -- the observers of the flow: derived fields, tracer particles, running flow
// statistics, wall loads.  Each reads the fields the step carries and writes only buffers of its own (ns_solver's dv,
// tr, av, lo: owned, so nothing here frees by hand); the step (ns_solver.cpp, step_body_) calls avg_sample,
// loads_sample and tracer_advance behind K1 and never reads what they leave.  One rank each.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ns_solver.h"

using namespace nss;

namespace {

// the entry prologue (ns_solver.h: enter) with each observer's words
int tracers_on(ns_solver* s, const char* who, int flags = 0) {
    return enter(s, who, s && s->tr.on, "tracers are not enabled", "ns_tracers_enable", flags);
}
int avg_on(ns_solver* s, const char* who, int flags = 0) {
    return enter(s, who, s && s->av.on, "flow statistics are not enabled", "ns_avg_enable", flags);
}
int loads_on(ns_solver* s, const char* who, int flags = 0) {
    return enter(s, who, s && s->lo.on, "wall loads are not enabled", "ns_loads_enable", flags);
}
int loads_edge(ns_solver* s, const char* who, int32_t edge) {
    CHK(loads_on(s, who));
    if (edge < 0 || edge >= s->n_edges) { set_err("%s: edge %d of a grid with %d edges", who, edge, s->n_edges); return NS_EINVAL; }
    return 0;
}

// ---------------- wall loads (ns_loads_enable; DESIGN.md 4 "Wall loads")
// the boundary faces' values and the edges' sums of the planes U, V, PHI (T) hold now, on the solver's stream: the face
// kernel, then (out != null) the edge sums into the record at out.  The geometry and the scalar's state are read per
// launch: an edge profile or a scalar enabled since the last one changes them.  No sync, no readback
int loads_run(ns_solver* s, double* out, bool timed) {
    auto& q = s->lo;
    nsg::LoadArgs& a = q.a;
    a.g = s->g;
    a.c = s->c;
    a.alpha = s->dt / (2 * s->re);
    a.re = s->re;
    a.u = s->arr[NS_ARR_U];
    a.v = s->arr[NS_ARR_V];
    a.phi = s->arr[NS_ARR_PHI];
    a.T = s->sc.on ? s->sc.T : nullptr;   // (the scalar's current plane: its sweeps swap T and its partner)
    a.pe = s->sc.on ? s->sc.pe : 1.0;
    for (int k = 0; k < 4; k++) {
        a.tneu[k] = s->sc.neu[k];
        a.tc[k] = s->sc.c[k];
    }
    {
        Timing::Scope iv;
        TCHK(s->tm.open(iv, nsg::T_LOADS, timed && s->timing));
        if (nsg::launch_load_faces(a, s->st) < 0) { set_err("wall loads: the face kernel's launch was refused"); return NS_EHIP; }
        TCHK(iv.close());
    }
    if (out) {
        Timing::Scope iv;
        TCHK(s->tm.open(iv, nsg::T_LOADS, timed && s->timing));
        if (nsg::launch_load_edges(a, out, s->st) < 0) { set_err("wall loads: the edge sums' launch was refused"); return NS_EHIP; }
        TCHK(iv.close());
    }
    return 0;
}

}  // namespace

// ---------------- tracer particles (ns_tracers_enable; DESIGN.md 4 "Tracers")
// one advance of the particles by dt in the planes U, V hold now (inside a step: u^n, v^n, which K1 leaves there in the
// deferred-K5 path too), on the solver's stream; count: the fates' counts and the largest live age reduced into the
// tracers' own slots behind it (no slot of the step's is touched, no host sync)
int nss::tracer_advance(ns_solver* s, double dt, bool count) {
    auto& q = s->tr;
    q.a.g = s->g;   // (an edge profile set since the last launch changes the geometry's table pointers)
    q.a.u = s->arr[NS_ARR_U];
    q.a.v = s->arr[NS_ARR_V];
    q.a.n = q.n;
    q.a.dt = dt;
    Timing::Scope iv;
    TCHK(s->tm.open(iv, nsg::T_TRACER, s->timing));
    const int nb = nsg::launch_tracer(q.a, count ? 2 : 1, s->st);
    if (nb < 0) { set_err("the tracer kernel's launch was refused"); return NS_EHIP; }
    TCHK(iv.close());
    double* part = q.part.get();
    if (count) nsg::launch_reduce_sum_min(part, nb, 3, q.scal.get(), part + 3 * (size_t)nb, nb, 1, q.scal.get() + 3, s->st);
    return 0;
}

// ---------------- running flow statistics (ns_avg_enable; DESIGN.md 4 "Flow statistics")
// one sample of the planes U, V (PHI, T) hold now into the running means and co-moment sums, on the solver's stream
// (inside a step: u^n, v^n, phi^n, T^n right behind K1, which leaves them there in the deferred-K5 path too).  The
// pressure first, by the derived fields' cell pass storing P only, into the statistics' own plane.  n and w are
// host-side: no sync, no readback
int nss::avg_sample(ns_solver* s) {
    auto& q = s->av;
    nsg::MomArgs& a = q.a;
    const bool has_t = (q.flags & NS_AVG_SCALAR) != 0, has_p = (q.flags & NS_AVG_PRESSURE) != 0;
    a.src[0] = s->arr[NS_ARR_U];
    a.src[1] = s->arr[NS_ARR_V];
    if (has_t) a.src[2] = s->sc.T;   // (the scalar's current plane: its sweeps swap T and its partner)
    if (has_p) {
        Timing::Scope iv;
        TCHK(s->tm.open(iv, nsg::T_AVG, s->timing));
        const int nb = nsg::launch_derived(s->k, s->g, s->c, s->dt / (2 * s->re), s->arr[NS_ARR_U], s->arr[NS_ARR_V],
                                           s->arr[NS_ARR_PHI], q.P, nullptr, nullptr, q.ppart.get(), s->st);
        if (nb < 0) { set_err("flow statistics: the pressure pass's launch was refused"); return NS_EHIP; }
        TCHK(iv.close());
        a.src[q.nsrc - 1] = q.P;
    }
    a.w = 1.0 / (double)(q.n + 1);
    Timing::Scope iv;
    TCHK(s->tm.open(iv, nsg::T_AVG, s->timing));
    if (nsg::launch_moments(a, q.nsrc, (q.flags & NS_AVG_SECOND) != 0, has_t, s->st) < 0) {
        set_err("flow statistics: the moments kernel's launch was refused");
        return NS_EHIP;
    }
    TCHK(iv.close());
    q.n++;
    return 0;
}

// one record appended to the wall loads' ring: `step` and the sums of the current planes
int nss::loads_sample(ns_solver* s, int64_t step) {
    auto& q = s->lo;
    const int64_t slot = q.total % q.capacity;
    CHK(loads_run(s, q.ring.get() + (size_t)slot * q.nrec, true));
    q.rstep[slot] = step;
    q.total++;
    return 0;
}

// every observer's memory, by assigning fresh states (the caller knows the stream has passed their last launch)
void nss::observers_free(ns_solver* s) {
    s->dv = ns_solver::Derived{};
    s->tr = ns_solver::Tracers{};
    s->av = ns_solver::Averages{};
    s->lo = ns_solver::Loads{};
}

extern "C" {

// ---------------- derived fields ("Derived fields"): P, vorticity, divergence, psi and the integrals of
// the current u, v, phi.  One cell pass (24 B/cell in, only the planes asked for out) + psi's two launches + one
// reduction, all on the solver's stream with buffers of its own, each allocated on first use
int ns_derive(ns_solver* s, const ns_derived* out, ns_derived_stats* st) {
    CHK(enter(s, "ns_derive"));
    if (!out && !st) { set_err("ns_derive: out and st are both NULL"); return NS_EINVAL; }
    if (s->nranks > 1) { set_err("ns_derive: nranks > 1 is not supported"); return NS_EINVAL; }
    CHK(prepare(s, SETTLE | LAUNCH));
    using D = ns_solver::Derived;
    auto& q = s->dv;
    const nsg::Geo& g = s->g;
    const ns_derived none{nullptr, nullptr, nullptr, nullptr};
    const ns_derived& o = out ? *out : none;
    const size_t pl = (size_t)g.nxl * g.ld * sizeof(double);
    q.ncap = nsg::derived_partials(g);
    q.ldv = (g.ny + 1 + 15) & ~15;
    if (!q.part) CHK(dev_alloc(s, q.part, (size_t)q.ncap * 9 * sizeof(double), false, "derived partials"));
    if (!q.scal) CHK(dev_alloc(s, q.scal, D::NSLOT * sizeof(double), true, "derived slots"));
    if (!q.hs) CHK(pinned_alloc(q.hs, D::NSLOT));
    if (o.p && !q.p) CHK(dev_alloc(s, q.p, pl, true, "pressure plane"));
    if (o.vort && !q.w) CHK(dev_alloc(s, q.w, pl, true, "vorticity plane"));
    if (o.div && !q.d) CHK(dev_alloc(s, q.d, pl, true, "divergence plane"));
    if (o.psi && !q.psi) CHK(dev_alloc(s, q.psi, (size_t)(g.nx + 1) * q.ldv * sizeof(double), true, "stream-function plane"));
    if (o.psi && !q.base) CHK(dev_alloc(s, q.base, (size_t)(g.nx + 1) * sizeof(double), false, "stream-function base"));
    if (o.psi && !q.ppart) CHK(dev_alloc(s, q.ppart, (size_t)(g.nx + 1) * 2 * sizeof(double), false, "stream-function partials"));
    Timing::Scope iv;
    TCHK(s->tm.open(iv, nsg::T_DERIVED, s->timing));
    const int nb = nsg::launch_derived(s->k, g, s->c, s->dt / (2 * s->re), s->arr[NS_ARR_U], s->arr[NS_ARR_V],
                                       s->arr[NS_ARR_PHI], o.p ? q.p.get() : nullptr, o.vort ? q.w.get() : nullptr,
                                       o.div ? q.d.get() : nullptr, q.part.get(), s->st);
    if (nb < 0) { set_err("ns_derive: the cell pass's launch was refused"); return NS_EHIP; }
    TCHK(iv.close());
    int np = 0;
    if (o.psi) {
        np = nsg::launch_psi(g, s->c, s->arr[NS_ARR_U], s->arr[NS_ARR_V], q.base.get(), q.psi.get(), q.ldv, q.ppart.get(), s->st);
        if (np < 0) { set_err("ns_derive: the stream function's launch was refused"); return NS_EHIP; }
    }
    nsg::launch_derived_reduce(q.part.get(), nb, q.ncap, q.ppart.get(), np, q.scal.get(), s->st);
    HIPCHK(hipMemcpyAsync(q.hs.get(), q.scal.get(), D::NSLOT * sizeof(double), hipMemcpyDeviceToHost, s->st));
    const size_t wb = (size_t)g.ny * 8, ldb = (size_t)g.ld * 8;
    if (o.p) HIPCHK(hipMemcpy2DAsync(o.p, wb, q.p.get(), ldb, wb, g.nxl, hipMemcpyDeviceToHost, s->st));
    if (o.vort) HIPCHK(hipMemcpy2DAsync(o.vort, wb, q.w.get(), ldb, wb, g.nxl, hipMemcpyDeviceToHost, s->st));
    if (o.div) HIPCHK(hipMemcpy2DAsync(o.div, wb, q.d.get(), ldb, wb, g.nxl, hipMemcpyDeviceToHost, s->st));
    if (o.psi)
        HIPCHK(hipMemcpy2DAsync(o.psi, (size_t)(g.ny + 1) * 8, q.psi.get(), (size_t)q.ldv * 8, (size_t)(g.ny + 1) * 8, g.nx + 1,
                                hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    ns_derived_stats r{};
    TCHK(s->tm.drain(nsg::tbit(nsg::T_DERIVED), &r));
    const double* h = q.hs.get();
    r.ke = 0.5 * h[0];
    r.enstrophy = 0.5 * h[1];
    r.div_l2 = std::sqrt(h[2]);
    r.div_max = -h[3];
    r.cfl = s->dt * -h[4];
    r.vort_min = h[5];
    r.vort_max = -h[6];
    r.p_min = h[7];
    r.p_max = -h[8];
    r.psi_min = o.psi ? h[9] : NAN;
    r.psi_max = o.psi ? -h[10] : NAN;
    if (st) *st = r;
    return 0;
}

// ---------------- tracer particles ("Tracers"): the entry points.  Planes, tables, partials and slots of
// their own
int ns_tracers_enable(ns_solver* s, int64_t capacity) {
    CHK(enter(s, "ns_tracers_enable"));
    if (s->tr.on) { set_err("ns_tracers_enable: tracers are already enabled"); return NS_EINVAL; }
    if (capacity <= 0) { set_err("ns_tracers_enable: capacity %lld is not positive", (long long)capacity); return NS_EINVAL; }
    if (s->nranks > 1) {
        set_err("ns_tracers_enable: nranks > 1 is not supported (particles would migrate between slabs)");
        return NS_EINVAL;
    }
    HIPCHK(hipSetDevice(s->device));
    using Q = ns_solver::Tracers;
    Q q;
    const nsg::Geo& g = s->g;
    // the faces from the spacings the solver holds, summed one by one: xf[i + 1] = xf[i] + hx[i]
    std::vector<double> hx, hy;
    CHK(host_spacings(s, hx, hy));
    auto faces = [](const std::vector<double>& h, std::vector<double>& f) {
        f.assign(h.size() + 1, 0.0);
        for (size_t i = 0; i < h.size(); i++) f[i + 1] = f[i] + h[i];
        for (double v : h)
            if (v != h[0]) return 0.0;
        return (double)h.size() / f.back();   // uniform: cells per unit length
    };
    const double rhx = faces(hx, q.xf), rhy = faces(hy, q.yf);
    const size_t cap = (size_t)capacity;
    CHK(dev_alloc(s, q.mem, cap * (5 * sizeof(double) + sizeof(int32_t)), true, "tracer planes"));
    std::vector<double> tab(q.xf);
    tab.insert(tab.end(), q.yf.begin(), q.yf.end());
    CHK(dev_upload(s, q.tab, tab, "tracer face tables"));
    CHK(dev_alloc(s, q.part, (size_t)nsg::tracer_blocks(capacity) * 4 * sizeof(double), false, "tracer partials"));
    CHK(dev_alloc(s, q.scal, Q::NSLOT * sizeof(double), true, "tracer slots"));
    CHK(pinned_alloc(q.hs, Q::NSLOT));
    nsg::TracerArgs& a = q.a;
    a.xf = q.tab.get();
    a.yf = a.xf + g.nx + 1;
    a.rhx = rhx;
    a.rhy = rhy;
    a.x = q.mem.get();
    a.y = a.x + cap;
    a.wu = a.y + cap;
    a.wv = a.wu + cap;
    a.age = a.wv + cap;
    a.st = reinterpret_cast<int32_t*>(a.age + cap);
    a.part = q.part.get();
    // the edges a particle leaves the domain through (the rest are walls): per side on a rectangle, per edge on a mask
    auto open_edge = [&](int e) { return s->eprof[e].type == NS_BC_NEUMANN || s->eprof[e].type == NS_BC_INLET_UNI; };
    if (g.fc) {
        for (int e = 0; e < (int)s->eprof.size() && e < nsg::MAX_EDGES; e++)
            if (open_edge(e)) a.exitm |= 1u << e;
    } else {
        for (int k = 0; k < 4; k++)
            if (open_edge(s->side_edge[k])) a.exitm |= 1u << k;
    }
    q.cap = capacity;
    q.on = true;
    s->tr = std::move(q);
    return 0;
}

int ns_tracers_add(ns_solver* s, const double* x, const double* y, int64_t n) {
    CHK(tracers_on(s, "ns_tracers_add"));
    auto& q = s->tr;
    if (n < 0 || (n > 0 && (!x || !y))) { set_err("ns_tracers_add: %lld seeds with a NULL coordinate array", (long long)n); return NS_EINVAL; }
    if (n > q.cap - q.n) {
        set_err("ns_tracers_add: %lld seeds on top of %lld exceed the capacity %lld", (long long)n, (long long)q.n, (long long)q.cap);
        return NS_EINVAL;
    }
    const int nx = s->g.nx, ny = s->g.ny;
    auto cell = [](const std::vector<double>& f, double v) {   // f[i] <= v < f[i + 1], or -1
        if (!(v >= 0.0 && v < f.back())) return -1;
        return (int)(std::upper_bound(f.begin(), f.end(), v) - f.begin()) - 1;
    };
    for (int64_t k = 0; k < n; k++) {
        if (!std::isfinite(x[k]) || !std::isfinite(y[k])) {
            set_err("ns_tracers_add: seed %lld (%g, %g) is not finite", (long long)k, x[k], y[k]);
            return NS_EINVAL;
        }
        const int i = cell(q.xf, x[k]), j = cell(q.yf, y[k]);
        if (i < 0 || i >= nx || j < 0 || j >= ny || (!s->cid.empty() && s->cid[(size_t)i * ny + j] < 0)) {
            set_err("ns_tracers_add: seed %lld (%g, %g) is not in a domain cell", (long long)k, x[k], y[k]);
            return NS_EINVAL;
        }
    }
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(s->device));
    const nsg::TracerArgs& a = q.a;
    const size_t nb = (size_t)n * sizeof(double);
    HIPCHK(hipMemcpyAsync(a.x + q.n, x, nb, hipMemcpyHostToDevice, s->st));
    HIPCHK(hipMemcpyAsync(a.y + q.n, y, nb, hipMemcpyHostToDevice, s->st));
    HIPCHK(hipMemsetAsync(a.wu + q.n, 0, nb, s->st));
    HIPCHK(hipMemsetAsync(a.wv + q.n, 0, nb, s->st));
    HIPCHK(hipMemsetAsync(a.age + q.n, 0, nb, s->st));
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.st + q.n), NS_TRACER_LIVE | 4, (size_t)n, s->st));   // (fresh)
    HIPCHK(hipStreamSynchronize(s->st));   // (the caller owns x, y)
    q.n += n;
    return 0;
}

int ns_tracers_get(ns_solver* s, int64_t first, int64_t n, double* x, double* y, double* age, int32_t* state) {
    CHK(tracers_on(s, "ns_tracers_get"));
    auto& q = s->tr;
    if (first < 0 || n < 0 || first > q.n || n > q.n - first) {
        set_err("ns_tracers_get: the range [%lld, %lld) is outside [0, %lld)", (long long)first, (long long)(first + n), (long long)q.n);
        return NS_EINVAL;
    }
    HIPCHK(hipSetDevice(s->device));
    const nsg::TracerArgs& a = q.a;
    const size_t nb = (size_t)n * sizeof(double);
    if (n > 0) {
        if (x) HIPCHK(hipMemcpyAsync(x, a.x + first, nb, hipMemcpyDeviceToHost, s->st));
        if (y) HIPCHK(hipMemcpyAsync(y, a.y + first, nb, hipMemcpyDeviceToHost, s->st));
        if (age) HIPCHK(hipMemcpyAsync(age, a.age + first, nb, hipMemcpyDeviceToHost, s->st));
        if (state) HIPCHK(hipMemcpyAsync(state, a.st + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->st));
    }
    HIPCHK(hipStreamSynchronize(s->st));
    if (state)
        for (int64_t k = 0; k < n; k++) state[k] &= 3;   // (without the fresh bit)
    return 0;
}

int ns_tracers_sample(ns_solver* s, double* u, double* v) {
    CHK(tracers_on(s, "ns_tracers_sample", SETTLE | LAUNCH));
    auto& q = s->tr;
    if (q.n == 0) return 0;
    if (!q.smp) CHK(dev_alloc(s, q.smp, (size_t)q.cap * 2 * sizeof(double), true, "tracer samples"));
    q.a.g = s->g;
    q.a.u = s->arr[NS_ARR_U];
    q.a.v = s->arr[NS_ARR_V];
    q.a.n = q.n;
    q.a.su = q.smp.get();
    q.a.sv = q.a.su + q.cap;
    if (nsg::launch_tracer(q.a, 0, s->st) < 0) { set_err("the tracer kernel's launch was refused"); return NS_EHIP; }
    const size_t nb = (size_t)q.n * sizeof(double);
    if (u) HIPCHK(hipMemcpyAsync(u, q.a.su, nb, hipMemcpyDeviceToHost, s->st));
    if (v) HIPCHK(hipMemcpyAsync(v, q.a.sv, nb, hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    return 0;
}

int ns_tracers_advance(ns_solver* s, double dt, int32_t steps) {
    CHK(tracers_on(s, "ns_tracers_advance"));
    if (!std::isfinite(dt)) { set_err("ns_tracers_advance: dt = %g is not finite", dt); return NS_EINVAL; }
    if (steps < 0) { set_err("ns_tracers_advance: steps = %d is negative", steps); return NS_EINVAL; }
    CHK(prepare(s, SETTLE | LAUNCH));
    if (s->tr.n == 0 || steps == 0) return 0;
    (void)s->tm.drop(nsg::tbit(nsg::T_TRACER));   // (an earlier advance's intervals nobody asked for)
    for (int k = 0; k < steps; k++) CHK(tracer_advance(s, dt, k == steps - 1));
    return 0;
}

int ns_tracers_reset(ns_solver* s) {
    CHK(tracers_on(s, "ns_tracers_reset"));
    HIPCHK(hipSetDevice(s->device));
    s->tr.n = 0;
    HIPCHK(hipMemsetAsync(s->tr.scal.get(), 0, ns_solver::Tracers::NSLOT * sizeof(double), s->st));
    (void)s->tm.drop(nsg::tbit(nsg::T_TRACER));
    return 0;
}

int ns_tracers_last(ns_solver* s, ns_tracer_stats* out) {
    CHK(tracers_on(s, "ns_tracers_last"));
    if (!out) { set_err("ns_tracers_last: out is NULL"); return NS_EINVAL; }
    HIPCHK(hipSetDevice(s->device));
    auto& q = s->tr;
    HIPCHK(hipMemcpyAsync(q.hs.get(), q.scal.get(), ns_solver::Tracers::NSLOT * sizeof(double), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    ns_tracer_stats r{};
    TCHK(s->tm.drain(nsg::tbit(nsg::T_TRACER), &r));
    r.n = q.n;
    r.live = (int64_t)q.hs[0];
    r.exited = (int64_t)q.hs[1];
    r.stuck = (int64_t)q.hs[2];
    r.age_max = r.live > 0 ? -q.hs[3] : 0.0;
    *out = r;
    return 0;
}

// ---------------- running flow statistics ("Flow statistics"): the entry points.  Planes and partials of
// their own
int ns_avg_enable(ns_solver* s, const ns_avg_desc* d) {
    CHK(enter(s, "ns_avg_enable"));
    if (!d) { set_err("ns_avg_enable: the descriptor is NULL"); return NS_EINVAL; }
    if (s->av.on) { set_err("ns_avg_enable: flow statistics are already enabled"); return NS_EINVAL; }
    if (d->every < 1) { set_err("ns_avg_enable: every = %d is less than 1", d->every); return NS_EINVAL; }
    const int known = NS_AVG_SECOND | NS_AVG_PRESSURE | NS_AVG_SCALAR;
    if (d->flags & ~known) { set_err("ns_avg_enable: unknown flag bits 0x%x", (unsigned)(d->flags & ~known)); return NS_EINVAL; }
    if (s->nranks > 1) { set_err("ns_avg_enable: nranks > 1 is not supported (the pressure comes from ns_derive, one rank)"); return NS_EINVAL; }
    if ((d->flags & NS_AVG_SCALAR) && !s->sc.on) {
        set_err("ns_avg_enable: NS_AVG_SCALAR needs a scalar (ns_scalar_enable first)");
        return NS_EINVAL;
    }
    HIPCHK(hipSetDevice(s->device));
    ns_solver::Averages q;
    const nsg::Geo& g = s->g;
    const bool second = d->flags & NS_AVG_SECOND, has_p = d->flags & NS_AVG_PRESSURE, has_t = d->flags & NS_AVG_SCALAR;
    // the planes kept, in the kernel's order: sources u, v, T, P; co-moments uu, vv, uv, TT, uT, vT, pp
    int mean_of[4] = {NS_AVG_U, NS_AVG_V, -1, -1}, co_of[7] = {-1, -1, -1, -1, -1, -1, -1};
    int nsrc = 2, nco = 0;
    if (has_t) mean_of[nsrc++] = NS_AVG_T;
    if (has_p) mean_of[nsrc++] = NS_AVG_P;
    if (second) {
        co_of[nco++] = NS_AVG_UU; co_of[nco++] = NS_AVG_VV; co_of[nco++] = NS_AVG_UV;
        if (has_t) { co_of[nco++] = NS_AVG_TT; co_of[nco++] = NS_AVG_UT; co_of[nco++] = NS_AVG_VT; }
        if (has_p) co_of[nco++] = NS_AVG_PP;
    }
    const size_t pl = (size_t)g.nxl * g.ld;
    q.nplanes = (size_t)nsrc + nco;
    CHK(dev_alloc(s, q.mem, (q.nplanes + (has_p ? 1 : 0)) * pl * sizeof(double), true, "flow statistics planes"));
    if (has_p) CHK(dev_alloc(s, q.ppart, (size_t)nsg::derived_partials(g) * 9 * sizeof(double), false, "flow statistics partials"));
    double* next = q.mem.get();
    for (int k = 0; k < nsrc; k++, next += pl) q.plane[mean_of[k]] = q.a.mean[k] = next;
    for (int k = 0; k < nco; k++, next += pl) q.plane[co_of[k]] = q.a.S[k] = next;
    q.P = has_p ? next : nullptr;
    q.a.nxl = g.nxl;
    q.a.ny = g.ny;
    q.a.ld = g.ld;
    q.every = d->every;
    q.flags = d->flags;
    q.nsrc = nsrc;
    q.on = true;
    s->av = std::move(q);
    return 0;
}

int ns_avg_reset(ns_solver* s) {
    CHK(avg_on(s, "ns_avg_reset"));
    HIPCHK(hipSetDevice(s->device));
    auto& q = s->av;
    HIPCHK(hipMemsetAsync(q.mem.get(), 0, q.nplanes * (size_t)s->g.nxl * s->g.ld * sizeof(double), s->st));
    q.n = q.steps = 0;
    (void)s->tm.drop(nsg::tbit(nsg::T_AVG));
    q.acc = ns_avg_stats{};
    return 0;
}

int ns_avg_sample(ns_solver* s) {
    CHK(avg_on(s, "ns_avg_sample", SETTLE | LAUNCH));
    return avg_sample(s);
}

int ns_avg_get(ns_solver* s, int which, double* plane) {
    CHK(avg_on(s, "ns_avg_get"));
    if (which < 0 || which >= NS_AVG_NUM) { set_err("ns_avg_get: unknown plane %d", which); return NS_EINVAL; }
    auto& q = s->av;
    if (!q.plane[which]) {
        set_err("ns_avg_get: plane %d is not accumulated by this solver (ns_avg_enable's flags 0x%x)", which, (unsigned)q.flags);
        return NS_EINVAL;
    }
    if (!plane) { set_err("ns_avg_get: the output plane is NULL"); return NS_EINVAL; }
    HIPCHK(hipSetDevice(s->device));
    const nsg::Geo& g = s->g;
    const size_t cells = (size_t)g.nxl * g.ny;
    if (q.n == 0) {   // (nothing sampled: every plane is 0, and there is no 1 / n)
        HIPCHK(hipStreamSynchronize(s->st));
        std::fill(plane, plane + cells, 0.0);
        return 0;
    }
    HIPCHK(hipMemcpy2DAsync(plane, (size_t)g.ny * 8, q.plane[which], (size_t)g.ld * 8, (size_t)g.ny * 8, g.nxl,
                            hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    if (which >= NS_AVG_UU) {   // the population covariance S / n: one multiplication by the host-formed 1 / n
        const double rn = 1.0 / (double)q.n;
        for (size_t k = 0; k < cells; k++) plane[k] *= rn;
    }
    return 0;
}

int ns_avg_last(ns_solver* s, ns_avg_stats* out) {
    CHK(avg_on(s, "ns_avg_last"));
    if (!out) { set_err("ns_avg_last: out is NULL"); return NS_EINVAL; }
    HIPCHK(hipSetDevice(s->device));
    auto& q = s->av;
    HIPCHK(hipStreamSynchronize(s->st));
    TCHK(s->tm.drain(nsg::tbit(nsg::T_AVG), &q.acc));
    ns_avg_stats r = q.acc;
    q.acc = ns_avg_stats{};
    r.n = q.n;
    r.steps = q.steps;
    *out = r;
    return 0;
}

// ---------------- wall loads ("Wall loads"): the entry points.  Buffers of their own
int ns_loads_enable(ns_solver* s, const ns_load_desc* d) {
    CHK(enter(s, "ns_loads_enable"));
    if (!d) { set_err("ns_loads_enable: the descriptor is NULL"); return NS_EINVAL; }
    if (s->lo.on) { set_err("ns_loads_enable: wall loads are already enabled"); return NS_EINVAL; }
    if (d->every < 1) { set_err("ns_loads_enable: every = %d is less than 1", d->every); return NS_EINVAL; }
    if (d->capacity < 1) { set_err("ns_loads_enable: capacity = %d is less than 1", d->capacity); return NS_EINVAL; }
    if (s->nranks > 1) { set_err("ns_loads_enable: nranks > 1 is not supported (the pressure comes from ns_derive, one rank)"); return NS_EINVAL; }
    HIPCHK(hipSetDevice(s->device));
    ns_solver::Loads q;
    const nsg::Geo& g = s->g;
    std::vector<double> hx, hy;
    CHK(host_spacings(s, hx, hy));
    // the topology as the kernels see it: a rectangle's sides, or the masked domain's code plane
    std::vector<int32_t> fc;
    if (g.fc) {
        fc.resize((size_t)g.nxl * g.ld);
        HIPCHK(hipMemcpy(fc.data(), g.fc, fc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    auto inside = [&](int i, int j) { return fc.empty() || (fc[(size_t)i * g.ld + j] & nsg::FC_IN) != 0; };
    auto edge_of = [&](int i, int j, int k) {
        if (fc.empty()) {
            const bool bnd = k == 0 ? i == 0 : k == 1 ? i == g.nx - 1 : k == 2 ? j == 0 : j == g.ny - 1;
            return bnd ? s->side_edge[k] : -1;
        }
        const int e = nsg::fc_edge(fc[(size_t)i * g.ld + j], k);
        return e == nsg::FC_INT ? -1 : e;
    };
    nsg::LoadList& L = q.list;
    if (!nsg::build_load_list(g.nx, g.ny, g.ld, s->n_edges, hx.data(), hy.data(), inside, edge_of, L) || L.face.empty()) {
        set_err("ns_loads_enable: the boundary-face list could not be built");
        return NS_EINVAL;
    }
    const size_t nf = L.face.size(), nch = L.chunk.size(), nrec = (size_t)s->n_edges * NS_LOAD_NUM;
    // one table block: faces | chunks (16 bytes each) | the edges' chunk offsets
    std::vector<int32_t> tab(4 * (nf + nch) + L.cs.size());
    std::memcpy(tab.data(), L.face.data(), nf * sizeof(nsg::LoadFace));
    std::memcpy(tab.data() + 4 * nf, L.chunk.data(), nch * sizeof(nsg::LoadChunk));
    std::memcpy(tab.data() + 4 * (nf + nch), L.cs.data(), L.cs.size() * sizeof(int32_t));
    CHK(dev_upload(s, q.tab, tab, "wall-load tables"));
    CHK(dev_alloc(s, q.val, 6 * nf * sizeof(double), true, "wall-load face values"));
    CHK(dev_alloc(s, q.part, nch * NS_LOAD_NUM * sizeof(double), true, "wall-load partials"));
    CHK(dev_alloc(s, q.ring, ((size_t)d->capacity + 1) * nrec * sizeof(double), true, "wall-load records"));
    q.a.face = reinterpret_cast<const nsg::LoadFace*>(q.tab.get());
    q.a.chunk = reinterpret_cast<const nsg::LoadChunk*>(q.tab.get() + 4 * nf);
    q.a.cs = q.tab.get() + 4 * (nf + nch);
    q.a.val = q.val.get();
    q.a.part = q.part.get();
    q.a.nf = (int)nf;
    q.a.nchunk = (int)nch;
    q.a.n_edges = s->n_edges;
    q.every = d->every;
    q.capacity = d->capacity;
    q.nrec = (int)nrec;
    q.rstep.assign((size_t)d->capacity, 0);
    q.on = true;
    s->lo = std::move(q);
    return 0;
}

int ns_loads_reset(ns_solver* s) {
    CHK(loads_on(s, "ns_loads_reset"));
    auto& q = s->lo;
    q.total = q.steps = 0;
    (void)s->tm.drop(nsg::tbit(nsg::T_LOADS));
    q.acc = ns_load_stats{};
    return 0;
}

int ns_loads_sample(ns_solver* s) {
    CHK(loads_on(s, "ns_loads_sample", SETTLE | LAUNCH));
    return loads_sample(s, -1);
}

int ns_loads_edges(ns_solver* s, double* out) {
    CHK(loads_on(s, "ns_loads_edges"));
    if (!out) { set_err("ns_loads_edges: out is NULL"); return NS_EINVAL; }
    CHK(prepare(s, SETTLE | LAUNCH));
    auto& q = s->lo;
    double* rec = q.ring.get() + (size_t)q.capacity * q.nrec;   // (the record behind the ring)
    CHK(loads_run(s, rec, false));
    HIPCHK(hipMemcpyAsync(out, rec, (size_t)q.nrec * sizeof(double), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    return 0;
}

int ns_loads_face_count(ns_solver* s, int32_t edge, int64_t* n) {
    CHK(loads_edge(s, "ns_loads_face_count", edge));
    if (!n) { set_err("ns_loads_face_count: n is NULL"); return NS_EINVAL; }
    *n = s->lo.list.fs[edge + 1] - s->lo.list.fs[edge];
    return 0;
}

int ns_loads_faces(ns_solver* s, int32_t edge, const ns_load_faces* out) {
    CHK(loads_edge(s, "ns_loads_faces", edge));
    if (!out) { set_err("ns_loads_faces: out is NULL"); return NS_EINVAL; }
    CHK(prepare(s, SETTLE | LAUNCH));
    auto& q = s->lo;
    const size_t f0 = (size_t)q.list.fs[edge], n = (size_t)q.list.fs[edge + 1] - f0, nf = q.list.face.size();
    if (out->s) std::copy(q.list.s.begin() + f0, q.list.s.begin() + f0 + n, out->s);
    if (out->ds) std::copy(q.list.ds.begin() + f0, q.list.ds.begin() + f0 + n, out->ds);
    double* const dst[6] = {out->p, out->tx, out->ty, out->un, out->tb, out->qn};
    if (n == 0 || std::all_of(dst, dst + 6, [](double* p) { return !p; })) return 0;
    CHK(loads_run(s, nullptr, false));
    for (int k = 0; k < 6; k++)
        if (dst[k]) HIPCHK(hipMemcpyAsync(dst[k], q.val.get() + k * nf + f0, n * sizeof(double), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    return 0;
}

int ns_loads_history(ns_solver* s, int64_t first, int64_t n, int64_t* step, double* rec) {
    CHK(loads_on(s, "ns_loads_history"));
    auto& q = s->lo;
    const int64_t held = std::min<int64_t>(q.total, q.capacity);
    if (first < 0 || n < 0 || first > held || n > held - first) {
        set_err("ns_loads_history: the range [%lld, %lld) is outside [0, %lld)", (long long)first, (long long)(first + n), (long long)held);
        return NS_EINVAL;
    }
    HIPCHK(hipSetDevice(s->device));
    const int64_t oldest = q.total - held;   // (sample number of the oldest record held; its slot: % capacity)
    for (int64_t k = 0; k < n; k++) {
        const int64_t slot = (oldest + first + k) % q.capacity;
        if (step) step[k] = q.rstep[slot];
        if (rec)
            HIPCHK(hipMemcpyAsync(rec + (size_t)k * q.nrec, q.ring.get() + (size_t)slot * q.nrec, (size_t)q.nrec * sizeof(double),
                                  hipMemcpyDeviceToHost, s->st));
    }
    HIPCHK(hipStreamSynchronize(s->st));
    return 0;
}

int ns_loads_last(ns_solver* s, ns_load_stats* out) {
    CHK(loads_on(s, "ns_loads_last"));
    if (!out) { set_err("ns_loads_last: out is NULL"); return NS_EINVAL; }
    HIPCHK(hipSetDevice(s->device));
    auto& q = s->lo;
    HIPCHK(hipStreamSynchronize(s->st));
    TCHK(s->tm.drain(nsg::tbit(nsg::T_LOADS), &q.acc));
    ns_load_stats r = q.acc;
    q.acc = ns_load_stats{};
    r.total = q.total;
    r.held = std::min<int64_t>(q.total, q.capacity);
    r.steps = q.steps;
    *out = r;
    return 0;
}

}  // extern "C"
