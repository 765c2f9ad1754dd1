// Host test of the kernel-timing recorder (navierstokessolver_amd/csrc/ns_timing.h) against a stub of the event
// calls: a virtual clock instead of a GPU.  tests/test_timing_host.py compiles and runs it under the sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ns_timing.h"

struct Stub {
    using Event = int;
    using Stream = int;
    static inline std::vector<double> at;   // per event: when it was recorded / stamped (-1: never)
    static inline int destroyed = 0, arm_a = -1, arm_b = -1;
    static inline double clock = 0.0;
    static int create(Event* e) { *e = (int)at.size(); at.push_back(-1.0); return 0; }
    static int destroy(Event) { destroyed++; return 0; }
    static int record(Event e, Stream) { at[e] = clock; return 0; }
    static int wait(Event e) { return at[e] >= 0 ? 0 : 1; }
    static int elapsed(float* ms, Event a, Event b) {
        if (at[a] < 0 || at[b] < 0) return 1;
        *ms = (float)(at[b] - at[a]);
        return 0;
    }
    static void arm(Event a, Event b) { arm_a = a; arm_b = b; }
    static bool disarm() { const bool p = arm_a >= 0; arm_a = arm_b = -1; return p; }
    // a kernel launch: 1 ms of dispatch latency, then `ms` of kernel, which takes the armed stamp if there is one
    static bool launch(double ms) {
        clock += 1.0;
        const bool took = arm_a >= 0;
        if (took) { at[arm_a] = clock; at[arm_b] = clock + ms; }
        arm_a = arm_b = -1;
        clock += ms;
        return took;
    }
};
using T = nsg::Timing<Stub>;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)

static int timed_launch(T& tm, nsg::TKind kind, double ms, int weight = 1, bool markers = false) {
    T::Scope iv;
    if (int e = tm.open(iv, kind, true, weight, markers)) return e;
    Stub::launch(ms);
    return iv.close();
}

// S's own kind lands in S and in no other struct; a drain into ns_stats releases its interval without counting it
template <class S>
static void observer(T& tm, nsg::TKind kind, double lat) {
    CHECK(nsg::towned<S>() == nsg::tbit(kind) && nsg::trows<S>().size() == 1);
    S own{};
    ns_stats st, zero;
    std::memset(&st, 0, sizeof st);
    std::memset(&zero, 0, sizeof zero);
    CHECK(timed_launch(tm, kind, 2.0, 3) == 0);
    CHECK(tm.drain(~nsg::tbit(kind), &own) == 0 && own.n_kernels == 0);   // (not in the mask: kept)
    CHECK(tm.drain(~0u, &own) == 0 && own.n_kernels == 3 && own.t_kernel_ms == 2.0 + lat);
    CHECK(tm.drain(~0u, &own) == 0 && own.n_kernels == 3);                // (released)
    own = S{};
    CHECK(timed_launch(tm, kind, 2.0) == 0 && timed_launch(tm, nsg::T_K1, 1.0) == 0);
    CHECK(tm.drain(~0u, &st) == 0 && st.n_rhs_kernels == 1 && st.t_rhs_kernel_ms == 1.0 + lat);
    st.n_rhs_kernels = 0;
    st.t_rhs_kernel_ms = 0.0;
    CHECK(std::memcmp(&st, &zero, sizeof st) == 0);                       // (no line of ns_stats took it)
    CHECK(tm.drain(~0u, &own) == 0 && own.n_kernels == 0 && own.t_kernel_ms == 0.0);
    // ... and another struct's kinds leave S alone
    CHECK(timed_launch(tm, nsg::T_HELM, 1.0) == 0 && timed_launch(tm, nsg::T_SCALAR_RHS, 1.0) == 0);
    CHECK(tm.drain(~0u, &own) == 0 && own.n_kernels == 0 && own.t_kernel_ms == 0.0);
}

static void observers(T& tm, double lat) {
    observer<ns_derived_stats>(tm, nsg::T_DERIVED, lat);
    observer<ns_tracer_stats>(tm, nsg::T_TRACER, lat);
    observer<ns_avg_stats>(tm, nsg::T_AVG, lat);
    observer<ns_load_stats>(tm, nsg::T_LOADS, lat);
    // every kind but T_RAW has exactly one owner (the header's static_assert, spelled out kind by kind)
    for (int k = 0; k < nsg::T_NKIND; k++) {
        const unsigned b = 1u << k;
        const int owners = !!(nsg::towned<ns_stats>() & b) + !!(nsg::towned<ns_scalar_stats>() & b) +
                           !!(nsg::towned<ns_derived_stats>() & b) + !!(nsg::towned<ns_tracer_stats>() & b) +
                           !!(nsg::towned<ns_avg_stats>() & b) + !!(nsg::towned<ns_load_stats>() & b);
        CHECK(owners == (k == nsg::T_RAW ? 0 : 1));
    }
    CHECK(nsg::trows<ns_stats>().size() == 11 && nsg::trows<ns_scalar_stats>().size() == 1);
}

static void run(bool stamped) {
    T tm;
    tm.stamped = stamped;
    const double lat = stamped ? 0.0 : 1.0;   // marker events also count the dispatch latency
    // open / close / drain by kind, the weight, an interval kept across drains of other kinds (K5)
    CHECK(timed_launch(tm, nsg::T_K5, 7.0) == 0);
    for (int step = 0; step < 3; step++) {
        CHECK(timed_launch(tm, nsg::T_K1, 5.0) == 0);
        CHECK(timed_launch(tm, nsg::T_HELM, 2.0) == 0);
        CHECK(timed_launch(tm, nsg::T_HELM, 4.0, 2) == 0);
        CHECK(timed_launch(tm, nsg::T_SWEEP, 3.0) == 0);
        CHECK(timed_launch(tm, nsg::T_RESTRICT, 1.0) == 0);
        ns_stats mg{}, st{};
        CHECK(tm.drain(nsg::T_MG, &mg) == 0);
        CHECK(mg.n_poisson_kernels == 1 && mg.t_poisson_kernel_ms == 3.0 + lat);
        CHECK(mg.n_restrict_kernels == 1 && mg.t_restrict_kernel_ms == 1.0 + lat);
        CHECK(mg.n_helm_kernels == 0 && mg.n_k5_kernels == 0 && mg.n_rhs_kernels == 0);
        CHECK(tm.drain(nsg::tbit(nsg::T_HELM) | nsg::tbit(nsg::T_K1), &st) == 0);
        CHECK(st.n_helm_kernels == 3 && st.t_helm_kernel_ms == 6.0 + 2 * lat);
        CHECK(st.n_rhs_kernels == 1 && st.t_rhs_kernel_ms == 5.0 + lat && st.n_k5_kernels == 0);
        CHECK(tm.drain(nsg::T_MG | nsg::tbit(nsg::T_HELM), &st) == 0 && st.n_helm_kernels == 3);   // (released)
    }
    ns_stats st{};
    CHECK(tm.drain(nsg::tbit(nsg::T_K5), &st) == 0 && st.n_k5_kernels == 1 && st.t_k5_kernel_ms == 7.0 + lat);
    // events are reused across steps: six intervals were the most alive at once
    CHECK(tm.events() == 12);
    // the direct solve's phases share one count; the scalar's line goes to its own stats; drop() counts nothing
    CHECK(timed_launch(tm, nsg::T_FPS_DCT, 1.0) == 0 && timed_launch(tm, nsg::T_FPS_TRI, 2.0, 1, true) == 0);
    CHECK(timed_launch(tm, nsg::T_FPS_IDCT, 3.0) == 0 && timed_launch(tm, nsg::T_SCALAR_RHS, 4.0) == 0);
    ns_scalar_stats ss{};
    st = ns_stats{};
    CHECK(tm.drain(nsg::T_FPS, &st) == 0 && tm.drain(nsg::tbit(nsg::T_SCALAR_RHS), &ss) == 0);
    CHECK(st.n_fps_solves == 1 && st.t_fps_dct_ms == 1.0 + lat && st.t_fps_idct_ms == 3.0 + lat);
    CHECK(st.t_fps_tri_ms == 3.0);   // (markers asked for: the latency counts in either mode)
    CHECK(ss.n_rhs_kernels == 1 && ss.t_rhs_kernel_ms == 4.0 + lat);
    CHECK(timed_launch(tm, nsg::T_BAND, 1.0) == 0 && tm.drop(~0u) == 0);
    st = ns_stats{};
    CHECK(tm.drain(~0u, &st) == 0 && st.n_band_kernels == 0);
    observers(tm, lat);
    {   // the empty interval: no launch took the stamp -- counted, (next to) no time, and the stamp is gone
        T::Scope iv;
        CHECK(tm.open(iv, nsg::T_BAND) == 0 && iv.close() == 0 && Stub::arm_a < 0);
        CHECK(tm.drain(nsg::tbit(nsg::T_BAND), &st) == 0 && st.n_band_kernels == 1 && st.t_band_kernel_ms == 0.0);
    }
    {   // an abandoned interval (an early return between open and close) leaves no stamp armed and no figure
        {
            T::Scope iv;
            CHECK(tm.open(iv, nsg::T_K1) == 0);
            CHECK((Stub::arm_a >= 0) == stamped);
        }
        CHECK(Stub::arm_a < 0 && Stub::arm_b < 0);
        CHECK(!Stub::launch(1.0));   // (the next launch, some other solver's, is not stamped)
        st = ns_stats{};
        CHECK(tm.drain(~0u, &st) == 0 && st.n_rhs_kernels == 0 && tm.events() == 12);
    }
    {   // a muted scope, and a site that is not timed: nothing opens
        T::Scope iv;
        tm.mute = true;
        CHECK(tm.open(iv, nsg::T_SWEEP) == 0 && Stub::arm_a < 0 && iv.close() == 0);
        tm.mute = false;
        CHECK(tm.open(iv, nsg::T_SWEEP, false) == 0 && Stub::arm_a < 0 && iv.close() == 0);
        CHECK(tm.drain(~0u, &st) == 0 && st.n_poisson_kernels == 0);
    }
    // growth needs no pre-sizing: 1000 intervals alive at once; their sum and the first-start-to-last-end span
    const double t0 = Stub::clock;
    for (int k = 0; k < 1000; k++) CHECK(timed_launch(tm, nsg::T_RAW, 2.0) == 0);
    double tot = 0.0, span = 0.0;
    CHECK(tm.events() == 2000 && tm.drain_raw(&tot, &span) == 0);
    CHECK(tot == 1000 * (2.0 + lat) && span == Stub::clock - t0 - (stamped ? 1.0 : 0.0));
    CHECK(tm.drain_raw(&tot, &span) == 0 && tot == 0.0 && span == 0.0);
    for (int k = 0; k < 1000; k++) CHECK(timed_launch(tm, nsg::T_SWEEP, 1.0) == 0);
    CHECK(tm.events() == 2000);
    const int before = Stub::destroyed;
    tm.destroy();
    CHECK(Stub::destroyed - before == 2000 && tm.events() == 0);
}

int main() {
    run(false);
    run(true);
    std::printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
