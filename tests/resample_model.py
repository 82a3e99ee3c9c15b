"""A float64 model of the polyphase FIR resampler, written from the formulas (helper module: no tests, no product code, no library).

The operation is y[j] = sum_k x[i_j + k] * t_j[k]: a windowed-sinc (or cubic / linear) kernel sampled at the output's fractional position, every
row of taps divided by its own sum, and an index / phase walk over the input (i += samp_inc, phase += samp_frac, carry into i when phase reaches
out_rate).  The taps stay real numbers here - nothing is quantised or rounded to the sample format - and every inner product is summed with
math.fsum over its float64 products, so the model's own rounding is a few 2^-53 of A (below) however long the filter is.

Per output sample the model returns, next to y, the quantities the tolerances of tests/test_audio_model.py are made of:
    A = sum_k |x_k| * sum_r |ic_r| |row_r[k]|      what a relative rounding error anywhere in the sum is relative to
    S = sum_k |x_k|                                what one unit of tap quantisation is multiplied by
    C = sum_r |ic_r|                               the blend weights' gain (1 for taps that are not blended)
Integer formats are real numbers in LSB.

Plan (the published design rules of the reference resampler, restated):
    rates reduced by their gcd; Kaiser: beta and the tap count from stop-band attenuation and transition bandwidth, the cut-off multiplied by
    the quality's downsample factor; when downsampling cut-off and tap count scaled by out/in; sinc methods: tap count rounded up to a multiple
    of 8; oversample halved while mult * out < in (mult = 2, 4, ...), times 11 for linear interpolation; filter mode auto: the full table when
    it is smaller than 1 MiB (bytes per sample * taps * phases), interpolated otherwise.
    Oversampled rows: row i holds the taps at x = -(n/2) + i / oversample, x + 1, ...  An output of phase p uses rows offset .. offset + 1 (+ 3):
    pos = p * oversample, offset = (oversample - 1) - pos // n_phases, frac = pos % n_phases, blended with the linear / cubic weights of
    frac / n_phases.  The methods cubic and linear evaluate their kernel directly at x = 1 - n/2 - p / n_phases.
    Outside its support the Kaiser window keeps its edge value (the reference clamps the square root's argument at 0); the model does the same,
    it is part of the filter the goldens were made with.
update() is not modelled."""
import math

import numpy as np

# quality -> (cutoff, downsample cutoff factor, stop-band attenuation dB, transition bandwidth), oversample; the qualities the tests use
KAISER_QUALITY = {0: (0.860, 0.96511, 60.0, 0.7), 4: (0.940, 0.97979, 85.0, 0.087), 6: (0.945, 0.99471, 100.0, 0.068), 10: (0.975, 1.0, 120.0, 0.0305)}
OVERSAMPLE_QUALITY = {0: 4, 4: 8, 6: 16, 10: 32}
BLACKMAN_QUALITY = {4: (48, 0.85)}                # taps, cutoff
BYTES = {"S16LE": 2, "S32LE": 4, "F32LE": 4, "F64LE": 8}
PREC = {"S16LE": 15, "S32LE": 31}                 # integer formats: full scale is 2^prec LSB
EPS = {"F32LE": 2.0 ** -24, "F64LE": 2.0 ** -53}
FULL_TABLE_LIMIT = 1 << 20


def bessel_i0(x):
    """I0(x) = sum_k ((x/2)^2)^k / (k!)^2, all terms positive; summed from the small end"""
    q = np.asarray(x, np.float64) ** 2 / 4.0
    terms = [np.ones_like(q)]
    for k in range(1, 80):
        terms.append(terms[-1] * q / (k * k))
    total = np.zeros_like(q)
    for t in reversed(terms):
        total = total + t
    return total


def sinc_part(x, fc):
    y = math.pi * np.asarray(x, np.float64)
    safe = np.where(y == 0.0, 1.0, y)
    return np.where(y == 0.0, fc, np.sin(safe * fc) / safe)


def kaiser_taps(x, n, fc, beta):
    w = 2.0 * x / n
    return sinc_part(x, fc) * bessel_i0(beta * np.sqrt(np.maximum(1.0 - w * w, 0.0)))


def blackman_nuttall_taps(x, n, fc):
    w = 2.0 * math.pi * x / n + math.pi
    return sinc_part(x, fc) * (0.3635819 - 0.4891775 * np.cos(w) + 0.1365995 * np.cos(2 * w) - 0.0106411 * np.cos(3 * w))


def cubic_taps(x, n, b, c):
    """the (b, c) family of piecewise cubics over a support of n taps"""
    a = np.abs(x * 4.0) / n
    inner = ((12.0 - 9.0 * b - 6.0 * c) * a ** 3 + (-18.0 + 12.0 * b + 6.0 * c) * a ** 2 + (6.0 - 2.0 * b)) / 6.0
    outer = ((-b - 6.0 * c) * a ** 3 + (6.0 * b + 30.0 * c) * a ** 2 + (-12.0 * b - 48.0 * c) * a + (8.0 * b + 24.0 * c)) / 6.0
    return np.where(a <= 1.0, inner, np.where(a <= 2.0, outer, 0.0))


def linear_taps(x, n):
    return float((n + 1) // 2 * 2 // 2) - np.abs(x)


class Plan:
    """the filter of one resampler: fmt "S16LE" / "S32LE" / "F32LE" / "F64LE"; method "nearest" / "linear" / "cubic" / "blackman-nuttall" / "kaiser";
    filter_mode "auto" / "full" / "interpolated"; interpolation "cubic" / "linear" (sinc methods only)"""

    def __init__(self, fmt, in_rate, out_rate, method="kaiser", quality=4, filter_mode="auto", interpolation="cubic"):
        self.fmt, self.method = fmt, method
        self.is_int = fmt in PREC
        g = math.gcd(in_rate, out_rate)
        self.in_rate, self.out_rate = in_rate // g, out_rate // g
        self.samp_inc, self.samp_frac = divmod(self.in_rate, self.out_rate)
        self.n_phases = self.out_rate
        self.nearest = method == "nearest" or self.in_rate == self.out_rate        # equal rates: every output is an input sample
        down = self.out_rate < self.in_rate
        sinc = method in ("kaiser", "blackman-nuttall")
        self.fc = self.beta = 0.0
        if method == "nearest":
            n = 2
        elif method == "linear":
            n = 2
        elif method == "cubic":
            n = 4
        elif method == "blackman-nuttall":
            n, self.fc = BLACKMAN_QUALITY[quality]
        else:
            fc, factor, att, tr_bw = KAISER_QUALITY[quality]
            self.fc = fc * factor if down else fc
            self.beta = 0.1102 * (att - 8.7) if att > 50 else (0.5842 * (att - 21) ** 0.4 + 0.07886 * (att - 21) if att >= 21 else 0.0)
            n = int((att - 8.0) / (2.285 * 2.0 * math.pi * tr_bw)) + 1
        if down and method != "nearest":
            self.fc = self.fc * self.out_rate / self.in_rate
            n = n * self.in_rate // self.out_rate
        if sinc:
            n = (n + 7) // 8 * 8
        self.n_taps = n
        self.latency = n // 2
        self.blend = interpolation if sinc else "none"
        oversample = 1
        if sinc:
            oversample, mult = OVERSAMPLE_QUALITY[quality], 2
            while oversample > 1 and mult * self.out_rate < self.in_rate:
                mult *= 2
                oversample //= 2
            if interpolation == "linear":
                oversample *= 11
        self.oversample = oversample
        if not sinc:
            self.mode = "full"
        elif filter_mode == "auto":
            small = self.out_rate <= oversample or BYTES[fmt] * n * self.out_rate < FULL_TABLE_LIMIT
            self.mode = "full" if small else "interpolated"
        else:
            self.mode = filter_mode
        self.rows = None
        if sinc:
            count = oversample + (4 if self.blend == "cubic" else 2)
            self.rows = np.stack([self.row(-(n // 2) + i / oversample) for i in range(count)])
        self.cache = {}

    def row(self, x0):
        """taps at x0, x0 + 1, ..., divided by their sum"""
        x = x0 + np.arange(self.n_taps, dtype=np.float64)
        if self.method == "kaiser":
            t = kaiser_taps(x, self.n_taps, self.fc, self.beta)
        elif self.method == "blackman-nuttall":
            t = blackman_nuttall_taps(x, self.n_taps, self.fc)
        elif self.method == "cubic":
            t = cubic_taps(x, self.n_taps, 1.0, 0.0)
        else:
            t = linear_taps(x, self.n_taps)
        return t / math.fsum(t.tolist())

    def weights(self, frac):
        """blend weights of rows offset .. for the position frac / n_phases between them"""
        x = frac / self.n_phases
        if self.blend == "linear":
            return np.array([x, 1.0 - x])
        # the reference writes the cubic's 1/6 and 1/3 as the float literals 0.16667f and 0.33333f in its float and double code; its integer code
        # divides by 6 and by 3
        c6, c3 = (1.0 / 6.0, 1.0 / 3.0) if self.is_int else (float(np.float32(0.16667)), float(np.float32(0.33333)))
        x2, x3 = x * x, x * x * x
        ic0 = c6 * (x3 - x)
        ic1 = x + 0.5 * (x2 - x3)
        ic3 = -c3 * x + 0.5 * x2 - c6 * x3
        return np.array([ic0, ic1, 1.0 - ic0 - ic1 - ic3, ic3])

    def taps(self, phase):
        """(t, a, C) of an output of this phase: the real taps, sum_r |ic_r| |row_r|, sum_r |ic_r|"""
        hit = self.cache.get(phase)
        if hit is not None:
            return hit
        if self.blend == "none":
            t = self.row(1.0 - self.n_taps // 2 - phase / self.n_phases)
            res = (t, np.abs(t), 1.0)
        else:
            pos = phase * self.oversample
            offset, frac = (self.oversample - 1) - pos // self.n_phases, pos % self.n_phases
            ic = self.weights(frac)
            rows = self.rows[offset: offset + len(ic)]
            res = (ic @ rows, np.abs(ic) @ np.abs(rows), float(np.abs(ic).sum()))
        if len(self.cache) < 4096:
            self.cache[phase] = res
        return res


class Result:
    """one buffer's output: y, A, S as [n_out][channels], C as [n_out]"""

    def __init__(self, y, A, S, C):
        self.y, self.A, self.S, self.C = y, A, S, C


class Resampler:
    """one stream.  wrong: None, or one of "phase" (the phase one step ahead), "window" (the window one frame ahead), "tap" (the last tap dropped) -
    deliberately wrong models, for the test that the tolerances tell them from the right one."""

    def __init__(self, plan, channels, wrong=None):
        self.plan, self.channels, self.wrong = plan, channels, wrong
        self.base = 0                                        # absolute frame number of self.x[0]
        self.x = np.zeros((plan.n_taps // 2 - 1, channels))  # the stream starts with a history of n/2 - 1 silent frames
        self.index, self.phase = 0, 0                        # where the next output's window starts, and its phase
        self.kept = self.x.shape[0]                          # frames still ahead of the window after the last buffer

    def total(self):
        return self.base + self.x.shape[0]

    def out_frames(self, n_in):
        """outputs of the next buffer of n_in frames: output j sits at index + (phase + j * in_rate) / out_rate and is made while that position,
        a fraction, is at most the last one a whole window fits behind"""
        p = self.plan
        room = self.total() + n_in - self.index - p.n_taps
        if room < 0 or room * p.out_rate < self.phase:
            return 0
        return (room * p.out_rate - self.phase) // p.in_rate + 1

    def resample(self, data, n_in):
        """data [n_in][channels] (None: silence) in the sample format -> Result"""
        p, ch = self.plan, self.channels
        n_out = self.out_frames(n_in)
        new = np.zeros((n_in, ch)) if data is None else np.asarray(data).astype(np.float64).reshape(n_in, ch)
        self.x = np.concatenate([self.x, new])
        y, A, S, C = np.zeros((n_out, ch)), np.zeros((n_out, ch)), np.zeros((n_out, ch)), np.ones(n_out)
        n = p.n_taps
        for j in range(n_out):
            idx, phase = self.index, self.phase
            if self.wrong == "phase":
                phase += 1
                if phase == p.n_phases:
                    idx, phase = idx + 1, 0
            if self.wrong == "window":
                idx += 1
            if p.nearest:
                y[j] = self.x[idx - self.base]
                A[j] = S[j] = np.abs(y[j])
            else:
                t, a, C[j] = p.taps(phase)
                if self.wrong == "tap":
                    t = t.copy()
                    t[-1] = 0.0
                w = self.x[idx - self.base: idx - self.base + n]
                if w.shape[0] < n:                           # (only a wrong model looks past the end)
                    w = np.concatenate([w, np.zeros((n - w.shape[0], ch))])
                for c in range(ch):
                    y[j, c] = math.fsum((w[:, c] * t).tolist())
                aw = np.abs(w)
                A[j], S[j] = a @ aw, aw.sum(axis=0)
            self.index += p.samp_inc
            self.phase += p.samp_frac
            if self.phase >= p.out_rate:
                self.phase -= p.out_rate
                self.index += 1
        drop = min(self.index, self.total()) - self.base      # frames behind the window are never read again
        if drop > 0:
            self.x, self.base = self.x[drop:], self.base + drop
        self.kept = max(0, self.total() - self.index)
        return Result(y, A, S, C)


def tolerance(plan, res):
    """the largest |got - y| that rounding explains, [n_out][channels], derived in DESIGN.md 11.7c.
    floats: (n_taps / 4 + 16) * eps * A - n_taps / 4 additions in each of the four accumulators; 16 for the tap's conversion to the format, the
    blend, the product and the three combining additions.
    integers, in LSB: 2^(1 - prec) * C * S + 8 - a unit of tap quantisation per tap through the blend's gain, twice where the blended tap is
    rounded again (full tables); 8 for the truncated row sums, the quantised blend weights and the final rounding.
    nearest: 0."""
    if plan.nearest:
        return np.zeros_like(res.y)
    if plan.is_int:
        prec = PREC[plan.fmt]
        assert (res.A < 2.0 ** prec).all(), "the model's integer bound holds below full scale only"
        return 2.0 ** (1 - prec) * res.C[:, None] * res.S + 8.0
    return (plan.n_taps / 4.0 + 16.0) * EPS[plan.fmt] * res.A
