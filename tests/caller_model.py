"""gmer_caller restated in Python (reference src/gmer_caller.c, src/genotypes.c, src/binomial.c, src/simplex.c,
src/utils.c:209-248): the yardstick of the caller's tests.

Doubles are Python floats; lgamma, log, exp, pow and the float functions come from this host's libm through ctypes
(math.lgamma is CPython's own implementation, not libm's, and math.log / math.exp raise where C returns inf or NaN), rand
from libc.  A `float` operation of the reference is the double operation rounded to float (F): for + - * / and sqrt of float
operands that is the float operation exactly.  run_cli replays main() byte for byte; likelihoods() also returns, per
genotype, the relative error bound the GPU tests allow."""
import ctypes
import ctypes.util
import math
import struct

import numpy as np

_m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_c = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
for _n in ("lgamma", "log", "exp", "sqrt"):
    getattr(_m, _n).restype, getattr(_m, _n).argtypes = ctypes.c_double, [ctypes.c_double]
_m.pow.restype, _m.pow.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]
for _n in ("logf", "expf", "sqrtf"):
    getattr(_m, _n).restype, getattr(_m, _n).argtypes = ctypes.c_float, [ctypes.c_float]
_c.rand.restype = ctypes.c_int
lgamma, log, exp, sqrt, pow_, logf, expf, sqrtf = _m.lgamma, _m.log, _m.exp, _m.sqrt, _m.pow, _m.logf, _m.expf, _m.sqrtf

RAND_MAX = 2147483647
MAX_PROD = 16384
N_GT = 15
GT = ["-", "A", "B", "AA", "AB", "BB", "AAA", "AAB", "BBA", "BBB", "AAAA", "AAAB", "BBBA", "AABB", "BBBB"]
# genotype j: (mean of count A, mean of count B); means: 0 l_viga, 1 lambda / 2, 2 lambda, 3 1.5 lambda, 4 2 lambda
MEANS = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (1, 3), (2, 2), (0, 4)]
EPS = 2.0 ** -52
ALLOWANCE = 16  # units of EPS x the largest term, for the device's lgamma and exp
TINY = 4 * 2.0 ** -1074  # a product below the normal range is rounded to multiples of 2^-1074, once per multiplication
DEFAULT_PARAMS = (0.0547219, 4.2603e-05, 0.014934, 0.985023, 0.0, 65.48, -0.6792684)


class Refused(Exception):
    """an input the drop-in refuses (the reference misreads it)"""


def F(x):
    """x rounded to float"""
    return struct.unpack("f", struct.pack("f", x))[0] if x == x and abs(x) <= 3.4028234663852886e38 else (x if x != x else math.copysign(math.inf, x))


_LFACT = None


def lfact_table():
    global _LFACT
    if _LFACT is None:
        t = [0.0] * MAX_PROD
        for i in range(1, MAX_PROD):
            t[i] = t[i - 1] + log(float(i))
        _LFACT = t
    return _LFACT


def log_factorial(v):
    t, dv, val = lfact_table(), float(v), 0.0
    while v >= MAX_PROD:
        val += log(dv)
        dv -= 1
        v -= 1
    return val + t[v]


def _combinations(n, k):
    if k == 0 or k == n:
        return exp(0.0)
    if k == 1:
        return exp(log(float(n)))
    sums = [0.0] * 5
    for i in range(1, 5):
        sums[i] = log(float(i))
        for j in range(2, i):
            sums[i] += log(float(j))
    return exp(sums[n] - sums[n - k] - sums[k])


def dbinom(x, n, p):
    if x == 0 and p == 0:
        return 1.0
    if x == n and p == 1:
        return 1.0
    return _combinations(n, x) * pow_(p, float(x)) * pow_(1 - p, float(n - x))


class Model:
    """what depends on the parameters alone: the 15 priors and, per mean, size, lgamma (size), log p, size x log (1 - p)
    (None where size <= 0 or mean <= 0: the density is 0).  The eight parameters are floats, promoted to double."""

    def __init__(self, l_viga, p_0, p_1, p_2, lam, size, size2, pB):
        l_viga, p_0, p_1, p_2, lam, size, size2, pB = [F(v) for v in (l_viga, p_0, p_1, p_2, lam, size, size2, pB)]
        self.params = (l_viga, p_0, p_1, p_2, lam, size, size2, pB)
        pb, pa = pB, 1 - pB
        p = [0.0] * N_GT
        p[0] = p_0
        p[1] = pa * p_1
        p[2] = pb * p_1
        p[3] = pa * pa * p_2
        p[4] = 2 * pa * pb * p_2
        p[5] = pb * pb * p_2
        p_lisa = 1 - p_0 - p_1 - p_2
        l1 = l2 = 0.0
        if p_lisa >= 0:
            l1 = (-1 + sqrtf(F(1 + 4 * p_lisa))) / 2
            l2 = l1 * l1
        p[6], p[9], p[7], p[8] = dbinom(3, 3, pa) * l1, dbinom(0, 3, pa) * l1, dbinom(2, 3, pa) * l1, dbinom(1, 3, pa) * l1
        p[10], p[14], p[11], p[13], p[12] = (dbinom(4, 4, pa) * l2, dbinom(0, 4, pa) * l2, dbinom(3, 4, pa) * l2, dbinom(2, 4, pa) * l2,
                                             dbinom(1, 4, pa) * l2)
        self.prior = p
        mu = [l_viga, lam / 2, lam, lam * 1.5, lam * 2]
        r = [size + size2 * l_viga, size + size2 * lam / 2, size + size2 * lam, size + size2 * lam * 1.5, size + size2 * lam * 2]
        self.terms = []
        for i in range(5):
            if r[i] <= 0 or mu[i] <= 0:
                self.terms.append(None)
                continue
            pr = mu[i] / (r[i] + mu[i])
            self.terms.append((r[i], lgamma(r[i]), log(pr), log(1 - pr) * r[i]))
        self._density = {}

    def density(self, k, m):
        """(dnbinom_mu of count k under mean m, the largest magnitude among 1 and its terms)"""
        key = (k, m)
        got = self._density.get(key)
        if got is None:
            t = self.terms[m]
            if t is None:
                got = (0.0, 0.0)
            else:
                r, lg_r, logp, c1 = t
                lg = lf = c = 0.0
                if k:
                    lg, lf = lgamma(k + r), log_factorial(k)
                    c = lg - lg_r - lf
                p0 = logp * k
                got = (exp(c + p0 + c1), max(1.0, abs(lg), abs(lf), abs(p0), abs(c1)))
            self._density[key] = got
        return got

    def likelihoods(self, ka, kb):
        """(a[15], rel[15]): the likelihoods and the relative bound of each: ALLOWANCE x EPS x the largest term, added over the two densities"""
        a, rel = [0.0] * N_GT, [0.0] * N_GT
        for j, (ma, mb) in enumerate(MEANS):
            (q0, b0), (q1, b1) = self.density(ka, ma), self.density(kb, mb)
            a[j] = q0 * q1 * self.prior[j]
            rel[j] = ALLOWANCE * EPS * (b0 + b1)
        return a, rel


def tolerance(a, rel):
    """the absolute error allowed for a likelihood: the relative bound times the model's value, and TINY.  TINY is not an
    allowance for the functions: a product q0 * q1 * p below 2^-1022 has no 52 fraction bits left -- each of its two
    multiplications rounds to a multiple of 2^-1074 -- so a bound relative to such a value (0 included, where it would allow
    nothing and could not be divided by) cannot be met by any arithmetic, the reference's included."""
    return rel * abs(a) + TINY


def call(a):
    """calc_run: (best index by a strict > scan from 0, sum in index order)"""
    best, top, s = 0, a[0], a[0]
    for j in range(1, N_GT):
        s += a[j]
        if a[j] > top:
            best, top = j, a[j]
    return best, s


def mlogl(model, pairs):
    """mlogL3 over (a, b) count pairs: (the sum, the absolute error allowed to a device sum of the same markers): the sum of
    the markers' bounds, a marker's bound being the largest relative bound among its 15 likelihoods (the relative error of
    a sum of non-negative terms is a weighted mean of theirs, and the error of its logarithm is that relative error)."""
    total, bound = 0.0, 0.0
    for ka, kb in pairs:
        a, rel = model.likelihoods(ka, kb)
        s = 0.0
        for v in a:
            s += v
        if s < 1e-30:
            s = 1e-30
        total += log(s)
        bound += max(rel)
    return -total, bound


# ------------------------------------------------------------------ the parameters as the simplex sees them

MIN_P = F(1.0 / 8192)
MAX_E = 0.25
ONE_M = F(1 - MIN_P)


def logit(p):
    return logf(F(p / F(1 - p)))


def logit_1(a):
    return F(1 / F(1 + expf(F(-a))))


def logit_clamped(p, lo, hi):
    if p <= lo:
        p = lo
    elif p >= hi:
        p = hi
    else:
        p = F(F(p - lo) / F(hi - lo))
    return logit(p)


def logit_1_clamped(a, lo, hi):
    a = logit_1(a)
    return F(lo + F(F(hi - lo) * a))


def unpack_params(x):
    return [logit_1_clamped(x[0], MIN_P, MAX_E), logit_1_clamped(x[1], MIN_P, ONE_M), logit_1_clamped(x[2], MIN_P, ONE_M),
            logit_1_clamped(x[3], MIN_P, ONE_M), expf(x[4]), x[5], F(-expf(x[6]))]


class Training:
    """the objective of a training, distanceL3 with optim_run (src/gmer_caller.c:845-914): per chunk of max (2000, ceil (n /
    threads)) markers its mlogL3 and the coverage penalty in float; the chunks' sums added in order"""

    def __init__(self, pairs, pB, lambda_est, nthreads, run):
        self.pairs, self.pB, self.lambda_est, self.lambda_sigma, self.run = pairs, pB, lambda_est, F(lambda_est / 4), run
        n = len(pairs)
        self.chunk = max(2000, (n + nthreads - 1) // nthreads)
        self.uniq, inv = np.unique(np.array([p[0] for p in pairs] + [p[1] for p in pairs], dtype=np.int64), return_inverse=True)
        self.ia, self.ib = inv[:n], inv[n:]

    def logs(self, model):
        """log (max (sum of the likelihoods, 1e-30)) of every marker: the densities once per distinct count, the products and
        the sums as numpy doubles (the same IEEE operations in the same order as Model.likelihoods), the logarithm by libm"""
        q = np.array([[model.density(int(k), m)[0] for k in self.uniq] for m in range(5)], dtype=np.float64)
        qa, qb = q[:, self.ia], q[:, self.ib]
        s = None
        with np.errstate(all="ignore"):
            for j, (ma, mb) in enumerate(MEANS):
                a = qa[ma] * qb[mb] * model.prior[j]
                s = a if s is None else s + a
        return [log(1e-30 if v < 1e-30 else float(v)) for v in s]

    def distance(self, x):
        l_viga, p_0, p_1, p_2, lam, size, size2 = v = unpack_params(x)
        logs = self.logs(Model(*v, self.pB))
        result = 0.0
        for first in range(0, len(logs), self.chunk):
            part = logs[first:first + self.chunk]
            s = 0.0
            for t in part:
                s += t
            s = -s
            d = F(self.lambda_est - lam)
            s += F(F(F(F(float(len(part))) * d) * d) / F(self.lambda_sigma * self.lambda_sigma))
            result += s
        if F(F(p_0 + p_1) + p_2) > 1:
            result = result + 10000 - F(100000 * F(F(F(1 - p_0) - p_1) - p_2))
        delta0 = F(size + F(F(size2 * lam) / 2))
        if delta0 < 0:
            result = result + 10000 + 100 * delta0
        delta1 = F(size + F(size2 * l_viga))
        if delta1 < 0:
            result = result + 10000 + 100 * delta1
        self.run.iterations.append("%.6f" % result)
        return F(result)


def downhill_simplex(x, dx, nruns, tr):
    """src/simplex.c:14-210 for 7 dimensions and 100 steps a run; x is updated in place"""
    nd, npt = 7, 8

    def at(p):
        x[:] = [F(v) for v in p]
        return tr.distance(x)

    y = [0.0] * npt
    y[0] = tr.distance(x)
    for run in range(nruns):
        mp = [list(x) for _ in range(npt)]
        for i in range(nd):
            for j in range(npt):
                mp[j][i] = x[i]
            mp[i][i] = F(mp[i][i] + dx[i] * (0.9 + 0.2 * _c.rand() / RAND_MAX) / (5 * run + 1))
        for j in range(npt):
            y[j] = at(mp[j])
        for _ in range(100):
            lo = 0
            hi, nhi = (0, 1) if y[0] > y[1] else (1, 0)
            for i in range(npt):
                if y[i] < y[lo]:
                    lo = i
                if y[i] > y[hi]:
                    nhi, hi = hi, i
                elif y[i] > y[nhi] and i != hi:
                    nhi = i
            pb = [0.0] * nd
            for i in range(npt):
                if i != hi:
                    for j in range(nd):
                        pb[j] = F(pb[j] + mp[i][j])
            pb = [F(v / 7) for v in pb]
            pr = [F(2.0 * pb[j] - mp[hi][j]) for j in range(nd)]
            ypr = at(pr)
            if ypr <= y[lo]:
                prr = [F(F(2 * pr[j]) + -1.0 * pb[j]) for j in range(nd)]
                yprr = at(prr)
                take, ytake = (prr, yprr) if ypr > yprr else (pr, ypr)
            elif ypr >= y[nhi]:
                if ypr < y[hi]:
                    mp[hi], y[hi] = list(pr), ypr
                prr = [F(F(0.5 * mp[hi][j]) + 0.5 * pb[j]) for j in range(nd)]
                yprr = at(prr)
                if yprr < y[hi]:
                    take, ytake = prr, yprr
                else:
                    pr = [F(0.5 * F(mp[hi][j] + mp[lo][j])) for j in range(nd)]
                    ypr = at(pr)
                    if ypr < y[hi]:
                        take, ytake = pr, ypr
                    else:
                        prr = [F(-mp[hi][j] + 2.0 * mp[lo][j]) for j in range(nd)]
                        yprr = at(prr)
                        if yprr < y[hi]:
                            take, ytake = prr, yprr
                        else:
                            xa = F(F(F(F(3 * y[hi]) - F(8 * ypr)) + F(6 * y[lo])) - yprr)
                            xb = F(F(y[hi] - F(2 * y[lo])) + yprr)
                            xc = F(-0.5 * y[hi] + F(F(8 * ypr) / 3) - F(2 * y[lo]) + F(yprr / 6))
                            xd = F(F(xb * xb) - F(F(4 * xa) * xc))
                            if xd > 0:
                                num = 0.5 * (-xb - sqrt(xd))
                                lmin = F(num / xa) if xa != 0 else (math.copysign(math.inf, num) * math.copysign(1.0, xa) if num != 0 else math.nan)
                                if math.isfinite(lmin):
                                    pr = [F(F(lmin * mp[hi][j]) + F(F(1 - lmin) * mp[lo][j])) for j in range(nd)]
                                else:
                                    pr = [F(F(0.5 * mp[hi][j]) + F(0.5 * mp[lo][j])) for j in range(nd)]
                                ypr = at(pr)
                            take, ytake = (pr, ypr) if ypr < y[hi] else (mp[lo], y[lo])
            else:
                take, ytake = pr, ypr
            mp[hi], y[hi] = list(take), ytake
        lo = 0
        for i in range(1, npt):
            if y[i] < y[lo]:
                lo = i
        x[:] = mp[lo]


# ------------------------------------------------------------------ the text

_SPACE = b" \t\n\v\f\r"


def strtol(buf, pos):
    """strtol (buf + pos, NULL, 10) on a text with a NUL behind it"""
    n = len(buf)
    while pos < n and buf[pos] in _SPACE:
        pos += 1
    neg = False
    if pos < n and buf[pos] in b"+-":
        neg = buf[pos] == 0x2d
        pos += 1
    v = 0
    while pos < n and 0x30 <= buf[pos] <= 0x39:
        v = v * 10 + buf[pos] - 0x30
        pos += 1
    v = min(v, (1 << 63) - (0 if neg else 1))
    return -v if neg else v


def split_line(buf, start, length, max_tokens=8):
    """src/utils.c:233-248: the offsets of up to max_tokens tokens of the line at `start`, parted by any byte < ' '"""
    tok, s = [], start
    while len(tok) < max_tokens and buf[s] != 0x0a:
        e = s
        tok.append(s)
        while e - start < length and buf[e] >= 0x20:
            e += 1
        s = e
        if buf[s] != 0x0a:
            s += 1
    return tok


def _u32(v):
    return v & 0xffffffff


def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def pair_median(buf, starts, idx):
    m6 = []
    for i in idx:
        tok = split_line(buf, starts[i], starts[i + 1] - starts[i])
        npairs = (len(tok) - 2) // 2
        s = 0
        for j in range(npairs):
            s = _u32(s + strtol(buf, tok[2 + 2 * j]))
            s = _u32(s + strtol(buf, tok[3 + 2 * j]))
        m6.append(_u32(s * 6) // npairs)
    hi, lo = (max(m6), min(m6)) if m6 else (0, 0xffffffff)
    med = _u32(lo + hi) // 2
    while hi > lo:
        above, below = sum(v > med for v in m6), sum(v < med for v in m6)
        equal = len(m6) - above - below
        if hi == lo + 1:
            if above > below + equal:
                med = hi
            break
        if above > below:
            if above - below < equal:
                break
            lo = med
        elif below > above:
            if below - above < equal:
                break
            hi = med
        else:
            break
        med = (lo + hi) // 2
    return med // 6


def poisson(k, lam):
    dk, p = float(k), exp(-lam)
    while k > 0 and p != 0:
        p *= lam
        p /= dk
        dk -= 1
        k -= 1
    return p


def parse_calls(buf, starts, idx, median):
    """[(line, a, b)]: of every line the pair whose sum lies nearest the median, counts cut to 16 bits"""
    calls = []
    for i in idx:
        tok = split_line(buf, starts[i], starts[i + 1] - starts[i])
        best = (0, 0, 0x7fffffff)
        for j in range((len(tok) - 2) // 2):
            a, b = _i32(strtol(buf, tok[2 + 2 * j])), _i32(strtol(buf, tok[3 + 2 * j]))
            delta = abs(_i32(a + b - median))
            if delta < best[2]:
                best = (a, b, delta)
        calls.append((i, best[0] & 0xffff, best[1] & 0xffff))
    return calls


def allele_freq(calls, order=None):
    ppb = npb = 0.0
    for i in (order if order is not None else range(len(calls))):
        _, c0, c1 = calls[i]
        if c0 + c1:
            ppb += F(F(float(c1)) / F(float(c0 + c1)))
            npb += 1
    return F(ppb / npb) if npb else 0.0


def training_set(set_size, subset):
    train = list(range(set_size))
    for i in range(subset):
        p = int(set_size * (_c.rand() / (RAND_MAX + 1.0)))
        train[i], train[p] = train[p], train[i]
    return train


def fmt2(x):
    if x != x:
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%.2f" % x


class Run:
    """One run of main (): .exit, .stdout (bytes), .stderr_lines (the lines that do not depend on -D), .iterations (the values
    of the "Iteration N delta" lines, as printed, whatever the debug level), .printed (every probability printed, before
    %.2f rounds it)"""

    def __init__(self, argv, text):
        self.out, self.stderr_lines, self.iterations, self.exit, self.printed = [], [], [], 0, []
        _c.srand(1)
        self.main(list(argv), text)
        self.stdout = "".join(self.out).encode("latin-1")

    def train(self, calls, max_training, nruns, v, mul, nthreads):
        """train_model; returns pB, v is updated in place"""
        ntrain = min(len(calls), max_training)
        train = training_set(len(calls), ntrain)[:ntrain]
        s = float(sum(calls[i][1] + calls[i][2] for i in train))  # (integers: exact in double either way)
        pB = allele_freq(calls, train)
        mean = s / ntrain
        if mean == 0:
            self.stderr_lines.append("No calls in training sample, aborting model optimization")
            return pB
        if v[4] == 0:
            v[4] = F(mul * mean)
        x = [logit_clamped(v[0], MIN_P, MAX_E), logit_clamped(v[1], MIN_P, ONE_M), logit_clamped(v[2], MIN_P, ONE_M),
             logit_clamped(v[3], MIN_P, ONE_M), logf(v[4]), v[5], logf(F(-v[6]))]
        dx = [F(p / 10) for p in x]
        tr = Training([(calls[i][1], calls[i][2]) for i in train], pB, v[4], nthreads, self)
        downhill_simplex(x, dx, nruns, tr)
        if self.debug:
            tr.distance(x)
        v[:] = unpack_params(x)
        return pB

    def genotypes(self, buf, starts, calls, v, pB, nalleles, pc, alt):
        model = Model(*v, pB)
        for line, c0, c1 in calls:
            a, _ = model.likelihoods(c0, c1)
            best, summa = call(a)
            p = starts[line]
            j = 0
            while buf[p + j] != 0x09 and j < 255 and p + j < len(buf) - 1:
                j += 1
            name = buf[p:p + j].split(b"\0")[0].decode("latin-1")
            can = nalleles == 0 or (nalleles == 1 and best in (1, 2)) or (nalleles == 2 and best in (3, 4, 5))
            if a[best] < pc or (not c0 and not c1):
                can = False
            shown = ([_div(a[best], summa)] if can else []) + ([_div(v_, summa) for v_ in a] if alt else [])
            self.printed += shown
            row = name + ("\t%s\t%s" % (GT[best], fmt2(shown[0])) if can else "\tNC\t") + "\t%d\t%d" % (c0, c1)
            if alt:
                row += "".join("\t" + fmt2(v_) for v_ in shown[-N_GT:])
            self.out.append(row + "\n")

    def main(self, argv, text):
        nruns, max_training, nthreads, header, non_canonical, pc = 5, 100000, 16, False, False, 0.0
        alt = info = False
        print_gt, model, params_given, fn, self.debug = True, "full", False, None, 0
        v = [F(p) for p in DEFAULT_PARAMS]
        i = 0
        while i < len(argv):
            a = argv[i]
            if a == "-D":
                self.debug += 1
            elif a in ("--runs", "--training_size", "--num_threads"):
                i += 1
                n = _u32(strtol(argv[i].encode() + b"\0", 0))
                if a == "--runs":
                    nruns = n
                elif a == "--training_size":
                    max_training = n
                else:
                    nthreads = n
            elif a == "--header":
                header = True
            elif a == "--non_canonical":
                non_canonical = True
            elif a == "--prob_cutoff":
                i += 1
                pc = F(float(argv[i]))
            elif a == "--model":
                i += 1
                model = argv[i]
            elif a == "--params":
                v = [F(float(s)) for s in argv[i + 1:i + 8]]
                params_given = True
                i += 7
            elif a == "--coverage":
                i += 1
                v[4] = F(float(argv[i]))
            elif a == "--alternatives":
                alt = True
            elif a == "--info":
                info = True
            elif a == "--no_genotypes":
                print_gt = False
            else:
                fn = a
            i += 1
        assert fn is not None and model in ("full", "diploid", "haploid") and 1 <= nthreads <= 32
        if model == "haploid" and not params_given:
            v[2], v[3] = F(0.985023), F(0.014934)
        if text.count(b"\n") < 1:
            self.stderr_lines.append("File contains no lines")
            self.exit = 1
            return
        if not text.endswith(b"\n"):
            raise Refused("no final newline")
        buf = text + b"\0"
        starts = [0] + [k + 1 for k in range(len(text)) if text[k] == 0x0a]
        nlines = len(starts) - 1
        groups = ([], [], [])
        for k in range(nlines):
            c = buf[starts[k]]
            if model != "full" or 0x30 < c <= 0x39:
                groups[0].append(k)
            elif c == 0x58:
                groups[1].append(k)
            elif c == 0x59:
                groups[2].append(k)
        for g in groups:
            for k in g:
                if len(split_line(buf, starts[k], starts[k + 1] - starts[k])) < 4:
                    raise Refused("line %d has fewer than 4 tokens" % (k + 1))
        a_idx, x_idx, y_idx = groups
        a_med = pair_median(buf, starts, a_idx)
        x_med = y_med = 0
        p_xx = p_x = p_y = p_1 = 0.0
        if model == "full":
            x_med, y_med = pair_median(buf, starts, x_idx), pair_median(buf, starts, y_idx)
            p_xx, p_x, p_y, p_1 = poisson(x_med, float(a_med)), poisson(x_med, float(a_med // 2)), poisson(y_med, float(a_med // 2)), poisson(y_med, 1.0)
            if (p_y > p_1) if p_xx > p_x else (p_y < p_1):
                self.stderr_lines.append("Y inconsistency: p_1 %g p_Y %g p_X %g p_XX %g" % (p_1, p_y, p_x, p_xx))
        female = p_xx > p_x
        calls_a = parse_calls(buf, starts, a_idx, a_med)
        if nruns and calls_a:
            pB = self.train(calls_a, max_training, nruns, v, 2 if model == "haploid" else 1, nthreads)
        else:
            pB = allele_freq(calls_a)
        if info:
            self.out.append("#gmer_counter version 4.2.16 (stable)\n")
            if model == "full":
                self.out.append("#Sex\t%s\n" % ("F" if female else "M"))
            self.out.append("#EstimatedCoverage\t%g\n#AverageMAF\t%g\n" % (v[4], pB))
            self.out.append("#AutosomeModel\t%s\n" % " ".join("%g" % p for p in v))
        xv = list(v)
        calls_x = []
        if model == "full":
            calls_x = parse_calls(buf, starts, x_idx, x_med)
            if calls_x and nruns and not female:
                xv[2], xv[3] = F(0.98), F(0.01)
                pB = self.train(calls_x, max_training, nruns, xv, 2, nthreads)
                if info:
                    self.out.append("#XModel\t%s\n" % " ".join("%g" % p for p in xv))
        if print_gt:
            if header:
                self.out.append("#ID\tGT\tPROB\tA_KMERS\tB_KMERS" + "".join("\t" + g for g in GT) + "\n")
            two, one = (0, 0) if non_canonical else (2, 1)
            self.genotypes(buf, starts, calls_a, v, pB, one if model == "haploid" else two, pc, alt)
            if model == "full":
                if female:
                    self.genotypes(buf, starts, calls_x, v, pB, two, pc, alt)
                else:
                    self.genotypes(buf, starts, calls_x, xv, pB, one, pc, alt)
                    self.genotypes(buf, starts, parse_calls(buf, starts, y_idx, y_med), xv, pB, one, pc, alt)


def _div(a, b):
    """a / b as C divides doubles"""
    if b == 0 and a == a:
        if a == 0:
            return -math.nan  # (0 / 0 makes this host's NaN: the sign bit set on x86-64)
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b if b != 0 else a


def run_cli(argv, text):
    return Run(argv, text)
