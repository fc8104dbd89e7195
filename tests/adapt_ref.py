"""An independent reference of the chain's warm-up adaptation (hmcmt_chain_adapt_*, include/hmcmt.h) in numpy's longdouble: the window
schedule, the dual averaging of the step size and the mass from a window by a two-pass variance.  It uses nothing of the library's --
neither its item functions nor its Python side -- and is written from the header's description, not from csrc/hmcmt_items.h."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def window_ends(nwarmup, init, term, base):
    """The window ends as steps completed (the 0-based step of a window's last sample + 1), by Stan's rule."""
    last = nwarmup - term - 1
    end, size, ends = init + base - 1, base, []
    while True:
        ends.append(end + 1)
        if end == last:
            return ends
        size *= 2
        nxt = end + size
        if nxt != last and nxt + 2 * size >= nwarmup - term:
            nxt = last
        end = nxt


def window_counts(nwarmup, init, term, base):
    """Samples per window: the first starts at step `init`, each later one behind the previous end."""
    ends = window_ends(nwarmup, init, term, base)
    return [e - s for s, e in zip([init] + ends[:-1], ends)]


def clip(dt, dt_min=0.0, dt_max=0.0):
    if dt_min > 0 and dt < dt_min:
        dt = LD(dt_min)
    if dt_max > 0 and dt > dt_max:
        dt = LD(dt_max)
    return dt


class DualAveraging:
    """x = ln dt in longdouble; restart(dt) at the begin call and behind a mass update, update(alpha) once per step."""

    def __init__(self, dt, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        self.delta, self.gamma, self.t0, self.kappa = LD(delta), LD(gamma), LD(t0), LD(kappa)
        self.restart(dt)

    def restart(self, dt):
        self.mu = np.log(LD(10) * LD(dt))
        self.s_bar = LD(0)
        self.x_bar = LD(0)
        self.x = np.log(LD(dt))
        self.t = 0

    def update(self, alpha):
        self.t += 1
        t = LD(self.t)
        eta = LD(1) / (t + self.t0)
        self.s_bar = (LD(1) - eta) * self.s_bar + eta * (self.delta - LD(alpha))
        self.x = self.mu - self.s_bar * np.sqrt(t) / self.gamma
        x_eta = t ** (-self.kappa)
        self.x_bar = (LD(1) - x_eta) * self.x_bar + x_eta * self.x
        return self.x

    def bound(self):
        """What a float64 evaluation of the recurrence may differ by in x and in x_bar at this update: s_bar carries a few ulps and
        is multiplied by sqrt(t) / gamma; the 8 inside covers mu and the average, the 8 in front a libm an ulp off in log, pow, sqrt."""
        return 8 * EPS * (float(np.sqrt(LD(max(self.t, 1)))) / float(self.gamma) + 8)


def alpha_of(hdif):
    """The acceptance probability the adaptation uses, from a record's hdif (float64, as the library forms it)."""
    with np.errstate(under="ignore"):
        return 1.0 if hdif > 0 else float(np.exp(np.float64(hdif)))


def window_mass(samples):
    """diag(M^-1) from a window's samples [ncell, n], n >= 2: (two-pass sample variance) * n / (n + 5) + 1e-3 * 5 / (n + 5), with w and f
    formed in float64 as the library's host forms them.  Returns (mass, n, mean, m2, w, f); mean and m2 in longdouble."""
    x = np.asarray(samples, dtype=np.float64).astype(LD)
    n = x.shape[1]
    if n < 2:
        raise ValueError("window_mass: a window of at least two samples")
    mean = x.sum(axis=1) / LD(n)
    dev = x - mean[:, None]
    m2 = (dev * dev).sum(axis=1)
    dn = np.float64(n)
    w, f = dn / (dn + 5.0), 1e-3 * 5.0 / (dn + 5.0)
    return (m2 / LD(n - 1)) * LD(w) + LD(f), n, mean, m2, float(w), float(f)


def mass_bound(mass, mean, m2, n, w):
    """Bound on |float64 mass - mass| per cell: the Welford variance to 16 eps max(|mean| / std, 1) relative (tests/chain_ref.py:
    moments_bounds, with the largest |mean| / std the cell's own), and 4 eps relative for the two roundings of var * w + f."""
    var = np.asarray(m2 / LD(n), dtype=np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(var > 0, np.maximum(np.abs(mean) / np.sqrt(var), 1.0), 1.0)
    return 16 * EPS * cond * var * (n / (n - 1.0)) * w + 4 * EPS * np.asarray(mass, dtype=np.float64)


class Warmup:
    """The whole adaptation replayed from what a chain returned: step(hdif, sample) once per successful step; .dt is the step size the
    next step uses (longdouble), .masses the list of (steps completed, mass, n, mean, m2, w) of the windows that updated the mass."""

    def __init__(self, dt, nwarmup, adapt_mass=True, init_buffer=75, term_buffer=50, base_window=25, delta=0.8, gamma=0.05, t0=10.0,
                 kappa=0.75, dt_min=0.0, dt_max=0.0):
        self.W, self.adapt_mass, self.init, self.term = int(nwarmup), bool(adapt_mass), int(init_buffer), int(term_buffer)
        self.da = DualAveraging(dt, delta, gamma, t0, kappa)
        self.dt_min, self.dt_max = dt_min, dt_max
        self.dt = LD(dt)
        self.c, self.active = 0, True
        self.ends = [e - 1 for e in window_ends(self.W, self.init, self.term, int(base_window))] if self.adapt_mass else []
        self.window, self.masses, self.closed = [], [], []

    def step(self, hdif, sample=None, alpha=None):
        """hdif: the record's (or None with alpha given, the acceptance probability itself)"""
        if not self.active:
            return self.dt
        alpha = alpha_of(hdif) if alpha is None else alpha
        in_window = self.adapt_mass and self.init <= self.c < self.W - self.term
        if in_window:
            self.window.append(np.array(sample, dtype=np.float64))
        self.dt = clip(np.exp(self.da.update(alpha)), self.dt_min, self.dt_max)
        if in_window and self.c in self.ends:
            n = len(self.window)
            self.closed.append((self.c + 1, n))
            if n >= 2:
                mass, n, mean, m2, w, f = window_mass(np.array(self.window).T)
                self.masses.append((self.c + 1, mass, n, mean, m2, w))
                self.da.restart(self.dt)
            self.window = []
        self.c += 1
        if self.c == self.W:
            if self.da.t > 0:
                self.dt = clip(np.exp(self.da.x_bar), self.dt_min, self.dt_max)
            self.active = False
        return self.dt

    def bound(self):
        """Bound on |ln(dt of the library) - ln(self.dt)| behind the step just made"""
        return self.da.bound()
