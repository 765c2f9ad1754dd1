"""The running flow statistics' normative statement in NumPy (ns_avg_*, k_moments; DESIGN.md 4, "Flow statistics").

Sample number n + 1 of a source plane x updates the stored planes with w = 1.0 / (n + 1), formed in double:

    dx   = x - xm            xm'  = xm + w * dx
    Sxx' = Sxx + dx * (x - xm')
    Sxy' = Sxy + dx * (y - ym')        # dx from x's old mean, ym' y's NEW mean

Stored: the means xm and the central co-moment sums S.  Handed out: the means as they stand and S * (1.0 / n), the
population covariances.  Co-moments kept: uu, vv, uv; with a pressure source pp; with a scalar source TT, uT, vT; no
others.  Every line below is one IEEE operation per NumPy operator (NumPy contracts nothing), and the device helper
is compiled with contraction off, so the kernel's planes are meant to be these bit for bit."""
import numpy as np

MEANS = ("u", "v", "p", "T")
# the co-moment S_ab: da (of a's old mean) * (b - b's new mean)
PAIRS = {"uu": ("u", "u"), "vv": ("v", "v"), "uv": ("u", "v"), "pp": ("p", "p"), "TT": ("T", "T"), "uT": ("u", "T"),
         "vT": ("v", "T")}
KEYS = MEANS + tuple(PAIRS)   # NS_AVG_U .. NS_AVG_VT, in order


class RunningStats:
    """The statement: sample(u=, v=[, p=][, T=]) per sample, result() as GpuSolver.averages() hands it out."""

    def __init__(self, shape, second=True, pressure=False, scalar=False):
        self.src = ["u", "v"] + (["p"] if pressure else []) + (["T"] if scalar else [])
        self.pairs = [k for k, (a, b) in PAIRS.items() if second and a in self.src and b in self.src]
        self.n = 0
        self.mean = {k: np.zeros(shape) for k in self.src}
        self.S = {k: np.zeros(shape) for k in self.pairs}

    def reset(self):
        self.n = 0
        for a in list(self.mean.values()) + list(self.S.values()):
            a[...] = 0.0

    def sample(self, **planes):
        assert sorted(planes) == sorted(self.src), (sorted(planes), self.src)
        w = 1.0 / (self.n + 1)
        x = {k: np.asarray(planes[k], dtype=np.float64) for k in self.src}
        d, new = {}, {}
        for k in self.src:
            d[k] = x[k] - self.mean[k]
            new[k] = self.mean[k] + w * d[k]
        for k in self.pairs:
            a, b = PAIRS[k]
            self.S[k] = self.S[k] + d[a] * (x[b] - new[b])
        self.mean = new
        self.n += 1

    def result(self):
        out = {k: self.mean[k].copy() for k in self.src}
        for k in self.pairs:
            out[k] = self.S[k] * (1.0 / self.n) if self.n > 0 else np.zeros_like(self.S[k])
        out["n"] = self.n
        return out


def two_pass(stack):
    """The definition: stack maps a source name to its (n, ...) samples; np.mean and the mean of the products of the
    deviations."""
    out = {k: np.mean(a, axis=0) for k, a in stack.items()}
    for k, (a, b) in PAIRS.items():
        if a in stack and b in stack:
            out[k] = np.mean((stack[a] - out[a]) * (stack[b] - out[b]), axis=0)
    return out


class StepDriver:
    """The bookkeeping of the time step in pure Python: step k since enable / reset (k = 0, 1, ..) with
    k % every == 0 samples the state the step starts from; sample_now() is ns_avg_sample."""

    def __init__(self, stats, every=1):
        assert every >= 1
        self.stats, self.every, self.steps = stats, every, 0
        self.sampled = []   # the step indices sampled since enable / reset (None: a sample_now)

    def step(self, **state):
        if self.steps % self.every == 0:
            self.stats.sample(**state)
            self.sampled.append(self.steps)
        self.steps += 1

    def sample_now(self, **state):
        self.stats.sample(**state)
        self.sampled.append(None)

    def reset(self):
        self.stats.reset()
        self.steps = 0
        self.sampled = []
