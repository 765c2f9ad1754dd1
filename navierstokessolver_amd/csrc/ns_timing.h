// ns_timing.h -- the one recorder of the step's kernel timings (host side; ns_solver owns one as `tm`).
//
// A timed call is an INTERVAL of a kind: opened before the call, closed after it, and later DRAINED by kind into
// the stats line of that kind (one row per kind, in the table of the struct that owns it, below).  Two modes, as
// ever: the dispatch-stamped single launch (`stamped`: one rank with k.ext_timing -- the next launch goes through hipExtLaunchKernel, which stamps
// the interval's events at the kernel's own begin and end; no launch = an empty interval) and marker events
// around the call, which also count the dispatch latency (slabs, NSGPU_EXT_TIMING=0, and the sites that ask for
// them: several launches or a library call in one interval).  Events are created on demand and reused.
// An interval left open -- an early return between open and close -- is cancelled by its Scope: the pending
// stamp is disarmed, so no later launch of this thread can take it.
// Api: the event calls (nsg::HipTiming in ns_internal.h; a stub in tests/timing_host_test.cpp).  Every int returned
// here is the Api's error code, 0 = success.
#pragma once
#include <array>
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

// one row per kind: the kind's (elapsed ms, weighted count) fields in the stats struct S that owns it; trows<S>() is
// S's table.  Every kind but T_RAW has exactly one owner (checked below).  A new timed line for a new struct: one enum
// value, one trows<> table beside these and the struct's name in the check's list -- no edit to Timing
template <class S>
struct TRow {
    TKind kind;
    double S::*t;
    int32_t S::*n;   // null: the line shares another's count
};
template <class S, size_t N>
using TRows = std::array<TRow<S>, N>;
template <class S>
constexpr auto trows() = delete;   // (a struct without a table owns no kind: it cannot be drained into)
template <> constexpr auto trows<ns_stats>() {
    return TRows<ns_stats, 11>{{
        {T_SWEEP, &ns_stats::t_poisson_kernel_ms, &ns_stats::n_poisson_kernels},
        {T_RESTRICT, &ns_stats::t_restrict_kernel_ms, &ns_stats::n_restrict_kernels},
        {T_CYCLE, &ns_stats::t_cycle_kernel_ms, &ns_stats::n_cycle_kernels},
        {T_GUESS, &ns_stats::t_guess_kernel_ms, &ns_stats::n_guess_kernels},
        {T_HELM, &ns_stats::t_helm_kernel_ms, &ns_stats::n_helm_kernels},
        {T_K1, &ns_stats::t_rhs_kernel_ms, &ns_stats::n_rhs_kernels},
        {T_BAND, &ns_stats::t_band_kernel_ms, &ns_stats::n_band_kernels},
        {T_K5, &ns_stats::t_k5_kernel_ms, &ns_stats::n_k5_kernels},
        // the direct solve's three phases share n_fps_solves: the recurrences, which every solve has, count it
        {T_FPS_DCT, &ns_stats::t_fps_dct_ms, nullptr},
        {T_FPS_TRI, &ns_stats::t_fps_tri_ms, &ns_stats::n_fps_solves},
        {T_FPS_IDCT, &ns_stats::t_fps_idct_ms, nullptr},
    }};
}
template <> constexpr auto trows<ns_scalar_stats>() { return TRows<ns_scalar_stats, 1>{{{T_SCALAR_RHS, &ns_scalar_stats::t_rhs_kernel_ms, &ns_scalar_stats::n_rhs_kernels}}}; }
template <> constexpr auto trows<ns_derived_stats>() { return TRows<ns_derived_stats, 1>{{{T_DERIVED, &ns_derived_stats::t_kernel_ms, &ns_derived_stats::n_kernels}}}; }
template <> constexpr auto trows<ns_tracer_stats>() { return TRows<ns_tracer_stats, 1>{{{T_TRACER, &ns_tracer_stats::t_kernel_ms, &ns_tracer_stats::n_kernels}}}; }
template <> constexpr auto trows<ns_avg_stats>() { return TRows<ns_avg_stats, 1>{{{T_AVG, &ns_avg_stats::t_kernel_ms, &ns_avg_stats::n_kernels}}}; }
template <> constexpr auto trows<ns_load_stats>() { return TRows<ns_load_stats, 1>{{{T_LOADS, &ns_load_stats::t_kernel_ms, &ns_load_stats::n_kernels}}}; }

// the kinds S owns, as a mask of tbit
template <class S>
constexpr unsigned towned() {
    unsigned m = 0;
    for (const TRow<S>& r : trows<S>()) m |= tbit(r.kind);
    return m;
}
// as many rows as kinds, and every kind but T_RAW in some row: each has exactly one owner
template <class... S>
constexpr bool one_owner_each() {
    return (trows<S>().size() + ...) == T_NKIND - 1 && (towned<S>() | ...) == (tbit(T_NKIND) - 1u) - tbit(T_RAW);
}
static_assert(one_owner_each<ns_stats, ns_scalar_stats, ns_derived_stats, ns_tracer_stats, ns_avg_stats, ns_load_stats>(),
              "a timed kind without an owner, or with two");

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

    // release the closed intervals of `kinds` (a mask of tbit); those whose kind S owns are first added, in interval
    // order, to their line of *st (null: nobody's figures -- drop).  The caller knows the stream has passed them
    template <class S>
    int drain(unsigned kinds, S* st) {
        int err = 0;
        for (size_t i = 0; i < iv_.size(); i++) {
            Iv& v = iv_[i];
            if (v.state != CLOSED || !(kinds >> v.kind & 1)) continue;
            for (const TRow<S>& r : trows<S>()) {
                if (!st || r.kind != v.kind) continue;
                float ms = 0.f;
                const int e = Api::elapsed(&ms, v.a, v.b);
                if (e && !err) err = e;
                if (!e) { st->*r.t += ms; if (r.n) st->*r.n += v.weight; }
            }
            release((int)i);
        }
        return err;
    }
    int drop(unsigned kinds) { return drain<ns_stats>(kinds, nullptr); }

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
        (void)drop(tbit(T_RAW));
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
