"""Exact-arithmetic routing networks: weights and inputs for which every engine mode is
exact, and an integer evaluator of the same networks.  Shared by test_routing_cpu.py and
test_routing_gpu.py; numpy only (torch only to hand out a state_dict).

Every Conv1d(64, 64, 3) is a router: an output channel has zero, one or two weights +-2^k at a
(cin, tap) drawn from np.random.default_rng(seed); stems carry small integer taps, BatchNorm is the
identity up to its fold residue (running_var = float32(1 - 1e-5)), every CBAM multiplies by exactly 1/4
(all of its weights zero) and the conv in front of it carries x4.  Inputs are k/16.  Every activation is
then a multiple of 1/16 below 94 (BUDGET), i.e. within 11 significant bits: exact in f16, in the f16 + e4m3
split (both lo planes zero), in split bf16 and in fp32.  The builder proves the bound while it draws the
weights: it runs the network on per-channel intervals for inputs in [-4/16, 32/16] and replaces a row that
would leave the budget by one that cannot.

One net() states each architecture once, over an engine E: _Builder draws the weights, _Ideal replays them
on int64 in units of 2^-24 with explicit gathers, shifts and adds.  Nothing here is shared with
oracle/models.py or the package; test_routing_cpu.py holds the two against each other.
"""
import copy
import functools

import numpy as np

ARCHS = ("DenoiseCNN", "RRCDNet", "DSDN", "ADSDN", "PIDN", "APIDN")
CBAM = ("ADSDN", "APIDN")
SIGMOID = ("PIDN", "APIDN")
N_BLOCKS = 15
# full receptive radius = number of conv layers on the longest path (dilated ones count twice); the
# fused kernels size their halos by it (csrc/common.hpp fused_halo; test_routing_cpu.py reads it there)
REACH = {"DenoiseCNN": 20, "RRCDNet": 29, "DSDN": 34, "ADSDN": 34, "PIDN": 32, "APIDN": 32}
FUSED_HALO = {a: REACH[a] for a in ("DenoiseCNN", "RRCDNet", "DSDN", "PIDN")}
# rows per tile of each geometry (test_routing_cpu.py holds these to the sources):
#   'f16' / 'f16-plain' tiles 640 (common.hpp H16_WB), 'f16-short' 256, the walk 576 positions per step;
#   fp32 / f16f8 / bf16x3 (fused_inplace.hip NetGeo): 128 * 5 = 640 everywhere but DSDN, 128 * 4 = 512;
#   CBAM team kernels: 512 rows (fp32 / f16f8 / bf16x3) and 640 (f16), 6 halo rows per side; CBAM segment
#   launches: 512 rows, halo = the segment's conv count (0, 1 or 2)
PINGPONG_ROWS, SHORT_ROWS, WALK_T = 640, 256, 576
INPLACE_ROWS = {"DenoiseCNN": 640, "RRCDNet": 640, "DSDN": 512, "PIDN": 640}
TEAM_ROWS, TEAM16_ROWS, TEAM_HALO = 512, 640, 6
SEGMENT_HALOS = (0, 1, 2)

X_LO, X_HI, X_SPIKE = -4, 20, 32          # inputs in units of 1/16: the plain range and the spike maximum
FRAC = 20                                 # the evaluator counts in units of 2^-(4 + FRAC)
BUDGET = 1500                             # |activation| bound in units of 1/16 (11 bits: 2047)
BN_VAR = np.float32(1 - 1e-5)


def nominal_T(arch, mode):
    """Most positions a tile of this path owns: rows minus the two halos."""
    if arch in CBAM:
        return (TEAM16_ROWS if mode == "f16" else TEAM_ROWS) - 2 * TEAM_HALO
    if mode.endswith("walk"):
        return WALK_T
    rows = PINGPONG_ROWS if mode in ("f16", "f16-plain") else SHORT_ROWS if mode == "f16-short" else INPLACE_ROWS[arch]
    return rows - 2 * FUSED_HALO[arch]


def path_T(arch, mode, L, segments=False):
    """The seam periods of this path at length L, a tuple: tiles own [i T, (i + 1) T).  One period per
    path, except: the f16 team kernel spreads L evenly over its ceil(L / 628) tiles (cbam.hip team_geo:
    T = ceil(L / TT)), and the CBAM segment fallback launches each segment with its own halo."""
    if arch in CBAM and segments:
        return tuple(TEAM_ROWS - 2 * h for h in SEGMENT_HALOS)
    T = nominal_T(arch, mode)
    if arch in CBAM and mode == "f16":
        TT = -(-L // T)
        T = -(-L // TT)
    return (T,)


def modes(arch):
    """The engine paths the GPU test drives on a network ('f16-short' / '-walk': forced tile geometries)."""
    m = ["fp32", "f16", "f16f8", "bf16x3"]
    if arch not in CBAM:
        m.insert(2, "f16-short")
        m.append("f16-walk")
    if arch == "RRCDNet":
        m += ["f16-plain", "f16-plain-walk"]
    return m


def gpu_lengths(arch, mode):
    """Tiny lengths, lengths around the receptive radius, three tiles and more with a ragged last one in
    every geometry (2049, 3001), and the last owned position exactly on a seam of this path's real tiling
    (2T, 2T + 1 for its nominal T; on the f16 team kernel 2T + 1 = 1257 becomes three even tiles of 419:
    a one-position last tile cannot occur there).  The in-place kernels on 640 rows pick their last
    tile's body by need = L - base + 2 rows (fused_inplace.hip IP_KERNEL: 2, 3, 4 or 5 blocks of 128): one
    more length, third tile, need = 450, runs the 4-block body that no other length here selects."""
    R, T = REACH[arch], nominal_T(arch, mode)
    Ls = {1, 2, 5, R, R + 1, 2 * R + 1, 2049, 3001, 2 * T, 2 * T + 1}
    if mode in ("fp32", "f16f8", "bf16x3") and INPLACE_ROWS.get(arch) == 640:
        Ls.add(2 * T - FUSED_HALO[arch] + 450 - 2)
    return sorted(Ls)


# ------------------------------------------------------------------------------------------------
# the six architectures, once, over an engine E (reference: */train.py forward of each network)
def net(arch, E):
    if arch == "DenoiseCNN":
        h = E.relu(E.stem("layers.0"))
        for i in range(2, 20):
            h = E.relu(E.route(h, f"layers.{i}.0"))
        return E.head(h, "layers.20")
    if arch == "RRCDNet":
        r = E.relu(E.stem("right_net.0", bn="right_net.1"))
        for i in range(3, 18):
            r = E.relu(E.route(r, f"right_net.{i}.0", bn=f"right_net.{i}.1"))
        r = E.head(r, "right_net.18", chain_k=1)
        h = E.relu(E.stem("left_net.0", bn="left_net.1"))
        for i in range(3, 10):
            h = E.relu(E.route(h, f"left_net.{i}.0", dil=2))
        h = E.relu(E.route(h, "left_net.10", bn="left_net.11"))
        for i in range(13, 19):
            h = E.relu(E.route(h, f"left_net.{i}.0", dil=2))
        left = E.head(h, "left_net.19", chain_k=1)
        return E.x_minus_half(r, left)
    if arch in ("DSDN", "ADSDN"):
        att = arch == "ADSDN"
        g = 2 if att else 0                                  # x4 in front of every CBAM
        if att:
            h = E.quarter(E.relu(E.stem("down_sampling.conv", gain=2)), "down_sampling.cbam")
        else:
            h = E.relu(E.stem("down_sampling.conv"))
        h = E.relu(E.route(h, "conv1"))
        h = E.relu(E.route(h, "conv2", gain=g, sparse=True, reserve=2 * N_BLOCKS))
        if att:
            h = E.quarter(h, "cbam")
        for i in range(N_BLOCKS):
            k = f"res_blocks.{i}"
            o = E.relu(E.route(h, k + ".conv1", bn=k + ".bn1"))
            o = E.route(o, k + ".conv2", bn=k + ".bn2", gain=g, resid=h, resid_relu=True)
            if att:
                o = E.quarter(o, k + ".cbam")
            h = E.relu(E.add(o, h))
        return E.head(h, "conv_out")
    if arch in ("PIDN", "APIDN"):
        att = arch == "APIDN"
        ident = E.relu(E.stem("down_sampling.0", reserve=2 * N_BLOCKS if att else 0))
        h = ident
        for i in range(N_BLOCKS):
            k = f"res_blocks.{i}"
            o = E.relu(E.route(h, k + ".0", bn=k + ".1"))
            if att:
                o = E.route(o, k + ".3", bn=k + ".4", gain=2, resid=h, resid_relu=False)
                h = E.add(E.quarter(o, k + ".5"), h)
            else:
                h = E.route(o, k + ".3", bn=k + ".4")
        return E.sigmoid(E.head(E.add(h, ident), "conv_out.0", logit_max=4))
    raise KeyError(arch)


# ------------------------------------------------------------------------------------------------
# builder: draws the weights while running the network on per-channel intervals (units of 1/16)
class _Sym:
    def __init__(self, lo, hi, cl, cr):
        self.lo, self.hi, self.cl, self.cr = np.asarray(lo, np.int64), np.asarray(hi, np.int64), cl, cr

    def bound(self):
        return np.maximum(-self.lo, self.hi)


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.layers = {}            # conv key -> record, in network order
        self.cbams = []
        self.reserved = []          # channels kept quiet for the chains' hops through a residual sum

    # -- stems: integer taps and bias; the two chain channels take x[t-1] + 1 and x[t+1] + 1 (> 0)
    def stem(self, key, bn=None, gain=0, reserve=0):
        """reserve: that many channels get negative taps only (at most 12/16 behind the ReLU) and are kept
        for the chains of the residual blocks to hop into."""
        rng = self.rng
        taps = np.zeros((64, 3), np.int64)
        bias = np.zeros(64, np.int64)                       # whole numbers
        cl, cr = (int(c) for c in rng.choice(64, 2, replace=False))
        self.reserved = [int(c) for c in rng.permutation(64) if c not in (cl, cr)][:reserve]
        for c in range(64):
            while True:
                t = rng.integers(-1, 3, 3)
                if 0 < np.abs(t).sum() <= 3:
                    break
            b = int(rng.integers(-1, 3))
            if c % 8 == 5 or c in self.reserved:           # negative taps: ReLU gives real zeros
                t, b = -np.abs(t), 0 if c in self.reserved else min(b, 0)
            taps[c], bias[c] = t, b
        taps[cl], bias[cl] = (1, 0, 0), 1
        taps[cr], bias[cr] = (0, 0, 1), 1
        bn_bias = rng.integers(-2, 3, 64) if bn else np.zeros(64, np.int64)     # /16
        bn_bias[[cl, cr]] = 0
        m = 1 << gain
        lo = (np.minimum(taps * X_LO, taps * X_SPIKE).clip(None, 0).sum(1) + 16 * bias + bn_bias) * m
        hi = (np.maximum(taps * X_LO, taps * X_SPIKE).clip(0, None).sum(1) + 16 * bias + bn_bias) * m
        assert max(-lo.min(), hi.max()) <= BUDGET * m
        self.layers[key] = dict(kind="stem", key=key, bn=bn, taps=taps * m, conv_bias=16 * bias * m,
                                bn_bias=bn_bias * m, chain=(cl, cr))
        return _Sym(lo, hi, cl, cr)

    def relu(self, a):
        return _Sym(a.lo.clip(0, None), a.hi.clip(0, None), a.cl, a.cr)

    def add(self, a, b):
        return _Sym(a.lo + b.lo, a.hi + b.hi, a.cl, a.cr)

    def quarter(self, a, key):
        assert not (a.lo % 4).any() and not (a.hi % 4).any()
        self.cbams.append(key)
        return _Sym(a.lo // 4, a.hi // 4, a.cl, a.cr)

    @staticmethod
    def _row_interval(a, row, bias):
        lo = hi = bias
        for cin, tap, sign, k in row:
            tl, th = min(int(a.lo[cin]), 0) << k, max(int(a.hi[cin]), 0) << k     # a padded tap reads 0
            lo, hi = (lo + tl, hi + th) if sign > 0 else (lo - th, hi - tl)
        return lo, hi

    def route(self, a, key, bn=None, dil=1, gain=0, resid=None, resid_relu=False, sparse=False, reserve=0):
        """One Conv1d(64, 64, 3) [+ BatchNorm1d] as a router.  gain: every weight and bias x 2^gain (the
        CBAM behind it gives it back).  resid: the tensor the result (/ 2^gain) is added to; the row is
        kept only if that sum stays inside the budget too.  The chain rows take the left / the right tap
        of the previous chain channel with weight 1 and no bias."""
        rng = self.rng
        m = 1 << gain
        quiet = resid is not None or sparse                 # mostly zero and -1 rows
        if resid is None:
            cl, cr = (int(c) for c in rng.choice(64, 2, replace=False))
        else:       # hop into two reserved channels: they hold next to nothing and nothing negative
            assert len(self.reserved) >= 2 and (resid.lo[self.reserved] >= 0).all(), key
            cl, cr = self.reserved[:2]
            self.reserved = self.reserved[2:]
        if reserve:
            self.reserved = [int(c) for c in rng.permutation(64) if c not in (cl, cr)][:reserve]
        rows, bias = [None] * 64, np.zeros(64, np.int64)
        lo, hi = np.zeros(64, np.int64), np.zeros(64, np.int64)
        for c in range(64):
            if c in (cl, cr):
                row, b = [(a.cl if c == cl else a.cr, 0 if c == cl else 2, 1, 0)], 0
            else:
                u = 0.0 if c in self.reserved else rng.random()
                p_zero, p_single = (0.45, 0.9) if quiet else (0.12, 0.75)
                if u < p_zero:
                    row = []
                else:
                    n = 1 if u < p_single else 2
                    ent = set()
                    while len(ent) < n:
                        ent.add((int(rng.integers(64)), int(rng.integers(3))))
                    neg = 0.7 if quiet else 0.25
                    row = [(ci, tp, -1 if rng.random() < neg else 1, int(rng.random() < 0.15) if n == 1 else 0)
                           for ci, tp in sorted(ent)]
                b = int(rng.integers(-2, 3)) if rng.random() < 0.4 and c not in self.reserved else 0
                if len(row) == 1 and row[0][2] < 0 and resid is None:
                    b = int(rng.integers(4, 24))            # relu(b - a): not an all-zero channel
            ok = False
            for attempt in (0, 1):
                l, h = self._row_interval(a, row, b)
                s_lo, s_hi = l, h
                if resid is not None:
                    s_lo, s_hi = l + int(resid.lo[c]), h + int(resid.hi[c])
                    if resid_relu:
                        s_lo, s_hi = max(s_lo, 0), max(s_hi, 0)
                if max(-l, h, -s_lo, s_hi) <= BUDGET:
                    ok = True
                    break
                assert c not in (cl, cr), (key, c)
                # fallback: cannot leave the budget if the input is inside it
                row, b = ([] if resid is not None else [(int(rng.integers(64)), int(rng.integers(3)), 1, 0)]), 0
            assert ok, (key, c)
            rows[c], bias[c], lo[c], hi[c] = row, b, l * m, h * m
        conv_bias = rng.integers(-1, 2, 64) * (bias != 0) if bn else bias.copy()
        self.layers[key] = dict(kind="route", key=key, bn=bn, dil=dil, gain=gain, rows=rows,
                                conv_bias=conv_bias * m, bn_bias=(bias - conv_bias) * m,
                                chain=(cl, cr), chain_in=(a.cl, a.cr))
        return _Sym(lo, hi, cl, cr)

    def head(self, a, key, chain_k=0, logit_max=None):
        """Conv1d(64, 1, 3): the two chains on the outer taps and three more +-2^k weights.  logit_max:
        all weights are scaled by 2^-s so that |z| <= logit_max for every input in range."""
        rng = self.rng
        row = [(a.cl, 0, 1, chain_k), (a.cr, 2, 1, chain_k)]
        used = {(a.cl, 0), (a.cr, 2)}
        quietest = [int(c) for c in np.argsort(a.bound(), kind="stable")[:24]]
        while len(row) < 5:
            ci, tp = int(rng.choice(quietest)), 1 if logit_max is None else int(rng.integers(3))
            if (ci, tp) not in used and ci not in (a.cl, a.cr):
                used.add((ci, tp))
                row.append((ci, tp, -1 if rng.random() < 0.5 else 1, int(rng.integers(-1, 2))))
        bias = int(rng.integers(-8, 9))                      # /16
        s = 0
        if logit_max is not None:
            mag = sum(int(a.bound()[ci]) << (k + 1) for ci, _, _, k in row)        # x2: k >= -1
            while mag > (2 * (16 * logit_max - abs(bias))) << s:
                s += 1
        row = [(ci, tp, sg, k - s) for ci, tp, sg, k in row]
        self.layers[key] = dict(kind="head", key=key, bn=None, row=row, bias=bias, scale=s, chain_in=(a.cl, a.cr))
        return None

    def x_minus_half(self, r, left):
        return None

    def sigmoid(self, z):
        return None


@functools.lru_cache(maxsize=None)
def _spec_cached(arch, seed):
    b = _Builder(seed)
    net(arch, b)
    return b.layers


def routing_spec(arch, seed):
    """conv key -> layer record, in network order; a copy the caller may perturb."""
    return copy.deepcopy(_spec_cached(arch, seed))


def big_layers(spec):
    return [k for k, r in spec.items() if r["kind"] == "route"]


def kstep(cin, tap):
    """One of the six K-steps of a big layer: tap x channel half."""
    return 2 * tap + (cin >= 32)


def spec_state_dict(spec, template):
    """Reference-format state_dict of a spec; template: conftest.golden_template(load_golden(arch))."""
    import torch
    sd = {}
    for rec in spec.values():
        key = rec["key"]
        if rec["kind"] == "stem":
            w = (rec["taps"].astype(np.float64))[:, None, :]
            b = rec["conv_bias"] / 16.0
        elif rec["kind"] == "route":
            w = np.zeros((64, 64, 3))
            for c, row in enumerate(rec["rows"]):
                for cin, tap, sign, k in row:
                    w[c, cin, tap] += sign * 2.0 ** (k + rec["gain"])
            b = rec["conv_bias"] / 16.0
        else:
            w = np.zeros((1, 64, 3))
            for cin, tap, sign, k in rec["row"]:
                w[0, cin, tap] += sign * 2.0 ** k
            b = np.array([rec["bias"] / 16.0])
        sd[key + ".weight"], sd[key + ".bias"] = w, np.asarray(b, np.float64)
        if rec["bn"]:
            bn = rec["bn"]
            sd[bn + ".weight"], sd[bn + ".running_mean"] = np.ones(64), np.zeros(64)
            sd[bn + ".running_var"] = np.full(64, BN_VAR, np.float32)
            sd[bn + ".bias"] = rec["bn_bias"] / 16.0
    out = {}
    for k, (shape, dt) in template.items():
        if k in sd:
            v = np.asarray(sd.pop(k))
            assert v.shape == shape, (k, v.shape, shape)
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v), k
            out[k] = torch.from_numpy(np.ascontiguousarray(v.astype(np.float32)))
        elif k.endswith("num_batches_tracked"):
            out[k] = torch.zeros(shape, dtype=dt)
        else:                                               # every CBAM tensor: zero
            assert any(p in k for p in ("cbam.", ".ca.", ".sa.")), k
            out[k] = torch.zeros(shape, dtype=dt)
    assert not sd, sorted(sd)
    return out


def routing_state_dict(arch, seed):
    from conftest import golden_template, load_golden
    return spec_state_dict(_spec_cached(arch, seed), golden_template(load_golden(arch)))


# ------------------------------------------------------------------------------------------------
# inputs
def routing_inputs(seed, n, L):
    """(n, L) float32 k/16, k in [-4, 20]: inside the hybrid's spike window [-0.3, 1.3]."""
    k = np.random.default_rng(1000 + seed).integers(X_LO, X_HI + 1, (n, L))
    return (k / 16.0).astype(np.float32)


def spiked_inputs(seed, n, L, rows=(1,)):
    """routing_inputs with a handful of positions of the spectra `rows` raised to (20, 32]/16: outside
    the spike window, below the input gate of 4."""
    x = routing_inputs(seed, n, L)
    rng = np.random.default_rng(2000 + seed)
    for r in rows:
        pos = rng.choice(L, min(L, 6), replace=False)
        x[r, pos] = rng.integers(X_HI + 1, X_SPIKE + 1, len(pos)) / 16.0
        x[r, pos[0]] = X_SPIKE / 16.0
    return x


# ------------------------------------------------------------------------------------------------
# the integer evaluator
def _shifted(a, off):
    """b[..., t] = a[..., t + off], zero outside."""
    L = a.shape[-1]
    b = np.zeros_like(a)
    if off == 0:
        b[...] = a
    elif 0 < off < L:
        b[..., :L - off] = a[..., off:]
    elif -L < off < 0:
        b[..., -off:] = a[..., :L + off]
    return b


def _scaled(a, k):
    if k >= 0:
        return a << k
    assert not (a & ((1 << -k) - 1)).any(), "inexact right shift"
    return a >> -k


def _bits(v):
    """bit length and number of trailing zeros of |v| (v != 0), elementwise."""
    m = np.abs(v)
    return np.frexp(m.astype(np.float64))[1], np.frexp((m & -m).astype(np.float64))[1] - 1


class _Ideal:
    ONE16 = 1 << FRAC                                       # 1/16 in evaluator units

    def __init__(self, spec, x):
        k = np.asarray(x, np.float64) * 16
        assert np.array_equal(k, np.round(k)), "inputs must be multiples of 1/16"
        self.spec = spec
        self.x = k.astype(np.int64) << FRAC                 # (n, L)
        self.max_abs, self.max_bits, self.max_units = 0.0, 0, 0
        self.logit = None

    def _note(self, a):
        """Significant bits of a tensor: the bit length of max|a| counted from the power of two that
        divides all of its elements (an upper bound on every single element's)."""
        m = np.abs(a)
        top = int(m.max())
        if top:
            low = int(np.bitwise_or.reduce(m.ravel()))
            self.max_bits = max(self.max_bits, (top // (low & -low)).bit_length())
            self.max_abs = max(self.max_abs, top / (16 << FRAC))
        return a

    def _units(self, mag, quantum_bits):
        """mag: a bound on the sum of |term| of every partial sum of a layer; quantum_bits: OR of numbers
        whose lowest set bit divides every term."""
        if quantum_bits:
            self.max_units = max(self.max_units, int(mag) // (quantum_bits & -quantum_bits))

    def stem(self, key, bn=None, gain=0, **_):
        rec = self.spec[key]
        n, L = self.x.shape
        out = np.zeros((n, 64, L), np.int64)
        for j in range(3):
            out += rec["taps"][None, :, j, None] * _shifted(self.x, j - 1)[:, None, :]
        b = (rec["conv_bias"] + rec["bn_bias"]) << FRAC
        out += b[None, :, None]
        tmax = int(np.abs(rec["taps"]).sum(1).max()) * int(np.abs(self.x).max())
        self._units(tmax + int(np.abs(b).max()), self.ONE16)
        return self._note(out)

    def relu(self, a):
        return np.maximum(a, 0)

    def add(self, a, b):
        return self._note(a + b)

    def quarter(self, a, key):
        return self._note(_scaled(_scaled(a, -1), -1))       # channel attention 1/2, spatial attention 1/2

    def route(self, a, key, bn=None, dil=1, gain=0, **_):
        rec = self.spec[key]
        out = np.zeros_like(a)
        # entries grouped by (tap, shift, which entry of its row): one gather per group, no output
        # channel twice in a group
        groups = {}
        for c, row in enumerate(rec["rows"]):
            assert len(row) <= 2
            for j, (cin, tap, sign, k) in enumerate(row):
                assert k + rec["gain"] >= 0
                groups.setdefault((tap, k, j), []).append((c, cin, sign))
        for (tap, k, _), ent in groups.items():
            cout, cin, sign = (np.array(v) for v in zip(*ent))
            t = _scaled(_shifted(a[:, cin], (tap - 1) * rec["dil"]), k + rec["gain"])
            out[:, cout] += sign[None, :, None] * t
        b = (rec["conv_bias"] + rec["bn_bias"]) << FRAC
        out += b[None, :, None]
        # a row has at most two terms, each at most max|a| << (1 + gain); every term is a multiple of
        # the power of two that divides all of a (weights are 2^k, k >= 0) and the biases
        amax, bmax = int(np.abs(a).max()), int(np.abs(b).max())
        low = int(np.bitwise_or.reduce(np.abs(a).ravel())) | int(np.bitwise_or.reduce(np.abs(b)))
        self._units(2 * (amax << (1 + rec["gain"])) + bmax, low)
        return self._note(out)

    def head(self, a, key, chain_k=0, logit_max=None):
        rec = self.spec[key]
        z = np.zeros_like(a[:, 0])
        mag = np.zeros_like(z)
        orbits = 0
        for cin, tap, sign, k in rec["row"]:
            t = _scaled(_shifted(a[:, cin], tap - 1), k)
            z += sign * t
            mag += np.abs(t)
            orbits |= int(np.bitwise_or.reduce(np.abs(t).ravel()))
        b = rec["bias"] << FRAC
        self._units((mag + abs(b)).max(), orbits | abs(b))
        return z + b

    def x_minus_half(self, r, left):
        y2 = 2 * self.x - r - left                           # 2 y
        assert np.abs(y2).max() < 1 << 52
        return y2.astype(np.float64) / (32 << FRAC)

    def sigmoid(self, z):
        self.logit = z.astype(np.float64) / (16 << FRAC)
        return 1.0 / (1.0 + np.exp(-self.logit))


def ideal_forward(arch, seed, x, spec=None):
    """Exact forward of the routing network (arch, seed) on x (n, L), multiples of 1/16; spec: a perturbed
    copy of routing_spec(arch, seed) to evaluate instead.  Returns a dict:
      y          float64; exact for the networks without a sigmoid head, the float64 sigmoid of the exact
                 logit otherwise
      logit      float64, exact; None without a sigmoid head
      max_abs    largest |activation| of any layer
      max_bits   most significant bits of any activation, counted per tensor from the power of two that
                 divides all of its elements
      max_units  a bound on the largest sum of |term| of any partial sum, in units of the power of two that
                 divides every term of its layer"""
    E = _Ideal(_spec_cached(arch, seed) if spec is None else spec, x)
    y = net(arch, E)
    if not isinstance(y, np.ndarray) or y.dtype != np.float64:
        assert np.abs(y).max() < 1 << 52
        y = y.astype(np.float64) / (16 << FRAC)
    return dict(y=y, logit=E.logit, max_abs=E.max_abs, max_bits=E.max_bits, max_units=E.max_units)


# ------------------------------------------------------------------------------------------------
# bars and the failure report
def bar(arch, ideal_y, delta):
    """The GPU tests' bar on max|y - ideal|; delta: the BatchNorm fold's residue of this network
    (test_routing_cpu.DELTA).  1DCNN: 0 (no BatchNorm, no sigmoid: every operation exact).  RRCDNet / DSDN /
    ADSDN: twice the residue plus one fp32 rounding of the output.  PIDN / APIDN: twice the residue plus
    expf and the division at 1-2 ulp each for outputs in (0, 1)."""
    if arch == "DenoiseCNN":
        return 0.0
    if arch in SIGMOID:
        return 2 * delta + 4 * 2.0 ** -24
    return 2 * delta + 2.0 ** -23 * max(1.0, float(np.abs(ideal_y).max()))


def describe_mismatch(y, ideal, tol, Ts, what=""):
    """'' if |y - ideal| <= tol everywhere (and y is finite); otherwise what a kernel author needs: how
    many positions are wrong, and for the first five the (spectrum, position), the position modulo each
    seam period of the path (Ts: path_T's tuple, or one int), its distance to the nearest seam and to L,
    and the error in units of 1/16."""
    y, ideal = np.asarray(y, np.float64), np.asarray(ideal, np.float64)
    Ts = (Ts,) if isinstance(Ts, int) else tuple(Ts)
    L = y.shape[-1]
    err = np.abs(y - ideal)
    bad = np.argwhere(~(err <= tol))                        # NaN counts as wrong
    if not bad.size:
        return ""
    lines = [f"{what}: {len(bad)} of {y.size} positions off by more than {tol:.3g} "
             f"(max {np.nanmax(err):.6g} = {np.nanmax(err) * 16:.4g}/16), L = {L}, T = {', '.join(map(str, Ts))}"]
    for n, p in bad[:5]:
        seams = "; ".join(f"p mod {T} = {p % T}, {min(p % T, T - p % T)} from a seam" for T in Ts)
        lines.append(f"  spectrum {n} position {p}: {seams}, {L - 1 - p} from the end; "
                     f"got {y[n, p]:.8g}, ideal {ideal[n, p]:.8g}, error {(y[n, p] - ideal[n, p]) * 16:+.6g}/16")
    return "\n".join(lines)
