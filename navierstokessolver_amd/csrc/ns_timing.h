// ns_timing.h -- the one recorder of the step's kernel timings (host side; ns_solver owns one as `tm`).
//
// A timed call is an INTERVAL of a kind: opened before the call, closed after it, and later DRAINED by kind into
// the stats line of that kind (one table row per kind, below).  Two modes, as ever: the dispatch-stamped single
// launch (`stamped`: one rank with k.ext_timing -- the next launch goes through hipExtLaunchKernel, which stamps
// the interval's events at the kernel's own begin and end; no launch = an empty interval) and marker events
// around the call, which also count the dispatch latency (slabs, NSGPU_EXT_TIMING=0, and the sites that ask for
// them: several launches or a library call in one interval).  Events are created on demand and reused.
// An interval left open -- an early return between open and close -- is cancelled by its Scope: the pending
// stamp is disarmed, so no later launch of this thread can take it.
// Api: the event calls (nsg::HipTiming in ns_internal.h; a stub in tests/timing_host_test.cpp).  Every int returned
// here is the Api's error code, 0 = success.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/nsgpu.h"

namespace nsg {

// one kind per stats line; T_RAW has none (ns_time_poisson*: drain_raw)
enum TKind : uint8_t { T_SWEEP, T_RESTRICT, T_CYCLE, T_GUESS, T_HELM, T_K1, T_BAND, T_K5, T_FPS_DCT, T_FPS_TRI,
                       T_FPS_IDCT, T_SCALAR_RHS, T_DERIVED, T_TRACER, T_AVG, T_LOADS, T_RAW, T_NKIND };
constexpr unsigned tbit(TKind k) { return 1u << k; }
constexpr unsigned T_MG = tbit(T_SWEEP) | tbit(T_RESTRICT) | tbit(T_CYCLE) | tbit(T_GUESS);
constexpr unsigned T_FPS = tbit(T_FPS_DCT) | tbit(T_FPS_TRI) | tbit(T_FPS_IDCT);

// kind -> (elapsed ms, weighted count) of ns_stats, of ns_scalar_stats, of ns_derived_stats, of ns_tracer_stats, of
// ns_avg_stats or of ns_load_stats.  A new timed line: one enum value, one row
struct TLine {
    double ns_stats::*t;
    int32_t ns_stats::*n;
    double ns_scalar_stats::*st;
    int32_t ns_scalar_stats::*sn;
    double ns_derived_stats::*dt = nullptr;
    int32_t ns_derived_stats::*dn = nullptr;
    double ns_tracer_stats::*pt = nullptr;
    int32_t ns_tracer_stats::*pn = nullptr;
    double ns_avg_stats::*at = nullptr;
    int32_t ns_avg_stats::*an = nullptr;
    double ns_load_stats::*lt = nullptr;
    int32_t ns_load_stats::*ln = nullptr;
};
inline const TLine& tline(TKind k) {
    static const TLine tab[T_NKIND] = {
        {&ns_stats::t_poisson_kernel_ms, &ns_stats::n_poisson_kernels, nullptr, nullptr},    // T_SWEEP
        {&ns_stats::t_restrict_kernel_ms, &ns_stats::n_restrict_kernels, nullptr, nullptr},  // T_RESTRICT
        {&ns_stats::t_cycle_kernel_ms, &ns_stats::n_cycle_kernels, nullptr, nullptr},        // T_CYCLE
        {&ns_stats::t_guess_kernel_ms, &ns_stats::n_guess_kernels, nullptr, nullptr},        // T_GUESS
        {&ns_stats::t_helm_kernel_ms, &ns_stats::n_helm_kernels, nullptr, nullptr},          // T_HELM
        {&ns_stats::t_rhs_kernel_ms, &ns_stats::n_rhs_kernels, nullptr, nullptr},            // T_K1
        {&ns_stats::t_band_kernel_ms, &ns_stats::n_band_kernels, nullptr, nullptr},          // T_BAND
        {&ns_stats::t_k5_kernel_ms, &ns_stats::n_k5_kernels, nullptr, nullptr},              // T_K5
        // the direct solve's three phases share n_fps_solves: the recurrences, which every solve has, count it
        {&ns_stats::t_fps_dct_ms, nullptr, nullptr, nullptr},                                // T_FPS_DCT
        {&ns_stats::t_fps_tri_ms, &ns_stats::n_fps_solves, nullptr, nullptr},                // T_FPS_TRI
        {&ns_stats::t_fps_idct_ms, nullptr, nullptr, nullptr},                               // T_FPS_IDCT
        {nullptr, nullptr, &ns_scalar_stats::t_rhs_kernel_ms, &ns_scalar_stats::n_rhs_kernels},   // T_SCALAR_RHS
        {nullptr, nullptr, nullptr, nullptr, &ns_derived_stats::t_kernel_ms, &ns_derived_stats::n_kernels},   // T_DERIVED
        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ns_tracer_stats::t_kernel_ms, &ns_tracer_stats::n_kernels},   // T_TRACER
        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ns_avg_stats::t_kernel_ms, &ns_avg_stats::n_kernels},   // T_AVG
        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ns_load_stats::t_kernel_ms, &ns_load_stats::n_kernels},   // T_LOADS
        {nullptr, nullptr, nullptr, nullptr},                                                // T_RAW
    };
    return tab[k];
}

template <class Api>
class Timing {
    enum : uint8_t { FREE, OPEN, CLOSED };
    struct Iv {
        typename Api::Event a, b;
        TKind kind;
        uint8_t state;
        bool stamp;      // this interval is the next launch's dispatch stamp
        int weight;
        uint64_t seq;    // opening order (drain_raw's span)
    };
    std::vector<Iv> iv_;
    std::vector<int> free_;
    uint64_t seq_ = 0;

    void release(int id) { iv_[id].state = FREE; free_.push_back(id); }

public:
    typename Api::Stream stream{};
    bool stamped = false;   // dispatch stamps where a site allows them; else marker events
    bool mute = false;      // a scope whose launches are not timed (a preconditioner's V-cycle): open() is a no-op

    // an interval while it is open; going out of scope open cancels it.  wait(): until its end event has passed
    class Scope {
        friend class Timing;
        Timing* t_ = nullptr;
        int id_ = -1;
        bool open_ = false;
    public:
        Scope() = default;
        Scope(const Scope&) = delete;
        Scope& operator=(const Scope&) = delete;
        ~Scope() { cancel(); }
        void cancel() {
            if (!open_) return;
            open_ = false;
            if (t_->iv_[id_].stamp) (void)Api::disarm();
            t_->release(id_);
        }
        int close() {
            if (!open_) return 0;
            Iv& v = t_->iv_[id_];
            int e = 0;
            if (!v.stamp) e = Api::record(v.b, t_->stream);
            else if (Api::disarm()) {   // no launch took the stamp: an empty interval
                e = Api::record(v.a, t_->stream);
                if (!e) e = Api::record(v.b, t_->stream);
            }
            if (e) { cancel(); return e; }
            open_ = false;
            v.state = CLOSED;
            return 0;
        }
        int wait() const { return t_ ? Api::wait(t_->iv_[id_].b) : 0; }
    };

    // open an interval of `kind` (nothing when !timed or muted); weight: what it adds to the kind's count;
    // markers: marker events even where dispatch stamps are on
    int open(Scope& sc, TKind kind, bool timed = true, int weight = 1, bool markers = false) {
        sc.cancel();
        sc.t_ = nullptr;
        if (!timed || mute) return 0;
        if (free_.empty()) {
            Iv v{};
            if (int e = Api::create(&v.a)) return e;
            if (int e = Api::create(&v.b)) { (void)Api::destroy(v.a); return e; }
            iv_.push_back(v);
            free_.push_back((int)iv_.size() - 1);
        }
        const int id = free_.back();
        Iv& v = iv_[id];
        v.kind = kind;
        v.weight = weight;
        v.stamp = stamped && !markers;
        if (v.stamp) Api::arm(v.a, v.b);
        else if (int e = Api::record(v.a, stream)) return e;
        free_.pop_back();
        v.seq = seq_++;
        v.state = OPEN;
        sc.t_ = this;
        sc.id_ = id;
        sc.open_ = true;
        return 0;
    }

    // add the closed intervals of `kinds` (a mask of tbit) to the stats (any may be null: those figures are
    // dropped) and release them.  The caller knows the stream has passed them
    int drain(unsigned kinds, ns_stats* st, ns_scalar_stats* sc = nullptr, ns_derived_stats* dv = nullptr,
              ns_tracer_stats* tr = nullptr, ns_avg_stats* av = nullptr, ns_load_stats* lo = nullptr) {
        int err = 0;
        for (size_t i = 0; i < iv_.size(); i++) {
            Iv& v = iv_[i];
            if (v.state != CLOSED || !(kinds >> v.kind & 1)) continue;
            const TLine& L = tline(v.kind);
            float ms = 0.f;
            if ((st && L.t) || (sc && L.st) || (dv && L.dt) || (tr && L.pt) || (av && L.at) || (lo && L.lt)) {
                const int e = Api::elapsed(&ms, v.a, v.b);
                if (e && !err) err = e;
                if (!e && st && L.t) { st->*L.t += ms; if (L.n) st->*L.n += v.weight; }
                if (!e && sc && L.st) { sc->*L.st += ms; sc->*L.sn += v.weight; }
                if (!e && dv && L.dt) { dv->*L.dt += ms; dv->*L.dn += v.weight; }
                if (!e && tr && L.pt) { tr->*L.pt += ms; tr->*L.pn += v.weight; }
                if (!e && av && L.at) { av->*L.at += ms; av->*L.an += v.weight; }
                if (!e && lo && L.lt) { lo->*L.lt += ms; lo->*L.ln += v.weight; }
            }
            release((int)i);
        }
        return err;
    }

    // the T_RAW intervals: the sum of their times, and the span from the first one's start to the last one's end
    int drain_raw(double* total_ms, double* span_ms) {
        int first = -1, last = -1, err = 0;
        *total_ms = *span_ms = 0.0;
        for (size_t i = 0; i < iv_.size(); i++) {
            Iv& v = iv_[i];
            if (v.state != CLOSED || v.kind != T_RAW) continue;
            float ms = 0.f;
            if (int e = Api::elapsed(&ms, v.a, v.b)) err = err ? err : e;
            *total_ms += ms;
            if (first < 0 || v.seq < iv_[first].seq) first = (int)i;
            if (last < 0 || v.seq > iv_[last].seq) last = (int)i;
        }
        float span = 0.f;
        if (first >= 0 && !err) err = Api::elapsed(&span, iv_[first].a, iv_[last].b);
        *span_ms = span;
        (void)drain(tbit(T_RAW), nullptr);
        return err;
    }

    size_t events() const { return 2 * iv_.size(); }   // created so far (tests)

    void destroy() {
        for (Iv& v : iv_) { (void)Api::destroy(v.a); (void)Api::destroy(v.b); }
        iv_.clear();
        free_.clear();
    }
    ~Timing() { destroy(); }
};

}  // namespace nsg
