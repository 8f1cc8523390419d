"""The premise of the exact-arithmetic routing networks (tests/routing_nets.py), pinned without a GPU:
the construction stays inside what every 16-bit mode represents exactly, the float64 reference forward
agrees with the integer evaluator up to the BatchNorm fold's residue, the two chains reach the last halo
row, and a wrong tap, channel or K-step moves the output by a whole input step."""
import functools

import numpy as np
import pytest
import torch

import routing_nets as rn
from conftest import golden_template, load_golden

SEEDS = (0, 1, 2)
LENGTHS = (1, 2, 5, 700, 2049)
DELTA_LENGTHS = LENGTHS + (3001,)         # the GPU test's longest


@functools.lru_cache(maxsize=None)
def _case(arch, seed, L, spiked):
    """(x, ideal_forward's result), computed once for the tests that share it."""
    x = rn.spiked_inputs(seed, 3, L) if spiked else rn.routing_inputs(seed, 3, L)
    x.setflags(write=False)
    return x, rn.ideal_forward(arch, seed, x)


# delta per network: max |oracle.models.FORWARD in float64 - ideal_forward|, the BatchNorm fold's residue
# (each folded scale is 1 + 1.7e-8), as test_reference_float64_agrees_with_ideal measures and prints it
# over seeds 0-2, both input generators and DELTA_LENGTHS; never measured from the engine.  The bars of
# the GPU test (routing_nets.bar) take these values from here.
#   measured: DenoiseCNN 0 (no BatchNorm), RRCDNet 6.116e-07, DSDN 1.281e-06, ADSDN 1.281e-06,
#   PIDN 4.427e-08 (logit 1.772e-07), APIDN 2.923e-08 (logit 1.233e-07); recorded rounded up to two digits
DELTA = {"DenoiseCNN": 0.0, "RRCDNet": 6.2e-7, "DSDN": 1.3e-6, "ADSDN": 1.3e-6, "PIDN": 4.5e-8, "APIDN": 3.0e-8}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("arch", rn.ARCHS)
def test_construction_keeps_its_premise(arch, seed):
    """<= 11 significant bits and |a| <= 512 on every activation, every partial sum below 2^24 units,
    spiked inputs within |x| <= 2; every tap and every K-step used, some all-zero rows."""
    for L in LENGTHS:
        for spiked in (False, True):
            x, r = _case(arch, seed, L, spiked)
            assert np.abs(x).max() <= 2.0 and x.min() >= -0.25
            assert r["max_bits"] <= 11, (L, r["max_bits"])
            assert r["max_abs"] <= 512, (L, r["max_abs"])
            assert r["max_units"] < 2 ** 24, (L, r["max_units"])
            assert np.isfinite(r["y"]).all()
            if arch in rn.SIGMOID:
                assert np.abs(r["logit"]).max() <= 4.0
    assert rn.routing_inputs(seed, 3, 2049).max() <= 1.25           # inside the spike window
    assert rn.spiked_inputs(seed, 3, 2049).max() == 2.0
    spec = rn.routing_spec(arch, seed)
    taps, ksteps, zero_rows = set(), set(), 0
    for key in rn.big_layers(spec):
        for row in spec[key]["rows"]:
            zero_rows += not row
            assert len(row) <= 2
            for cin, tap, sign, k in row:
                taps.add(tap)
                ksteps.add(rn.kstep(cin, tap))
    assert taps == {0, 1, 2} and ksteps == set(range(6)) and zero_rows > 0
    y = _case(arch, seed, 2049, False)[1]["y"]
    assert np.ptp(y) > (0.05 if arch in rn.SIGMOID else 1.0)          # not a degenerate output


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("arch", rn.ARCHS)
def test_state_dict_loads_and_folds_to_one_bit(arch, seed):
    """Reference keys, shapes and dtypes; every folded weight the package will see, w * gamma /
    sqrt(float32(var) + 1e-5) in float64 rounded to f16, is exactly +-2^k (or 0)."""
    sd = rn.routing_state_dict(arch, seed)
    tmpl = golden_template(load_golden(arch))
    assert list(sd) == list(tmpl)
    for k, (shape, dt) in tmpl.items():
        assert tuple(sd[k].shape) == shape and sd[k].dtype == dt, k
    spec = rn.routing_spec(arch, seed)
    for key, rec in spec.items():
        w = sd[key + ".weight"].numpy().astype(np.float64)
        if rec["bn"]:
            g = sd[rec["bn"] + ".weight"].numpy().astype(np.float64)
            var = sd[rec["bn"] + ".running_var"].numpy()
            assert var.dtype == np.float32
            w = w * (g / np.sqrt(var.astype(np.float64) + 1e-5))[:, None, None]
        if rec["kind"] == "stem":
            continue                                         # fp32 on the device: integer taps
        with np.errstate(over="raise", under="raise"):
            h = w.astype(np.float16).astype(np.float64)
        nz = h[h != 0]
        assert np.count_nonzero(h) == np.count_nonzero(w)
        assert (np.frexp(np.abs(nz))[0] == 0.5).all(), key
        if not rec["bn"]:
            assert np.array_equal(h, w), key
    for k, v in sd.items():                                  # CBAM: both attentions sigmoid(0)
        if any(p in k for p in ("cbam.", ".ca.", ".sa.")):
            assert not v.any(), k


@pytest.mark.parametrize("arch", rn.ARCHS)
def test_module_loads_the_state_dict_strictly(arch):
    """The drop-in module takes the routing state_dict with strict=True, and its eager fp32 forward on the
    CPU (the reference forward on the module's own submodules) meets the bar the GPU test holds the engine
    to: the arithmetic really is exact in fp32 (1DCNN: bitwise)."""
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(rn.routing_state_dict(arch, 0), strict=True)
    m.eval()
    x, r = _case(arch, 0, 700, True)
    with torch.no_grad():
        y = m(torch.from_numpy(x.copy()).unsqueeze(1)).squeeze(1).numpy()
    assert y.dtype == np.float32
    assert rn.describe_mismatch(y, r["y"], rn.bar(arch, r["y"], DELTA[arch]), 700, f"{arch} eager fp32") == ""
    if arch == "DenoiseCNN":
        assert np.array_equal(y, r["y"])


def _oracle64(arch, sd, x):
    from oracle.models import FORWARD
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        return FORWARD[arch](sd64, torch.from_numpy(np.asarray(x, np.float64)).unsqueeze(1)).squeeze(1).numpy()


@pytest.mark.parametrize("arch", rn.ARCHS)
def test_reference_float64_agrees_with_ideal(arch):
    """oracle.models.FORWARD in float64 on the routing state_dict against the integer evaluator: the
    distance is the BatchNorm fold's residue, delta (measured here from the reference against the ideal,
    never from the engine); on PIDN / APIDN also on the logit."""
    worst = worst_rel = worst_z = 0.0
    for seed in SEEDS:
        sd = rn.routing_state_dict(arch, seed)
        for L in DELTA_LENGTHS:
            for spiked in (False, True):
                x, r = _case(arch, seed, L, spiked)
                y = _oracle64(arch, sd, x)
                assert y.shape == r["y"].shape
                d = np.abs(y - r["y"]).max()
                worst, worst_rel = max(worst, d), max(worst_rel, d / max(np.abs(r["y"]).max(), 1e-30))
                if arch in rn.SIGMOID:
                    worst_z = max(worst_z, np.abs(np.log(y / (1 - y)) - r["logit"]).max())
    print(f"{arch}: delta = {worst:.3e} (relative to max|y| {worst_rel:.3e}; logit {worst_z:.3e}); "
          f"recorded {DELTA[arch]:.3e}")
    assert worst <= DELTA[arch]
    assert worst_z <= 64 * DELTA[arch]                     # 1 / (y (1 - y)) <= 57 for |z| <= 4
    if arch == "DenoiseCNN":
        assert worst == 0.0


@functools.lru_cache(maxsize=None)
def _source_geometry():
    """The tile geometry as the sources state it (csrc/common.hpp, fused_inplace.hip, cbam.hip)."""
    import os
    import re
    from conftest import PKG_DIR

    def src(name):
        with open(os.path.join(PKG_DIR, "csrc", name)) as f:
            return f.read()

    def const(text, name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))

    def macro(text, name):
        return int(re.search(r"#define " + name + r" (\d+)", text).group(1))

    common, inplace, cbam = src("common.hpp"), src("fused_inplace.hip"), src("cbam.hip")
    body = re.search(r"constexpr int fused_halo\(int arch\) \{\s*return (.*?);", common, re.S).group(1)
    names = {"DENOISECNN": "DenoiseCNN", "RRCDNET": "RRCDNet", "DSDN": "DSDN", "PIDN": "PIDN"}
    halo = {names[a]: int(v) for a, v in re.findall(r"arch == (\w+) \? (\d+)", body)}
    nbk = re.search(r"template <int ARCH> struct NetGeo \{ static constexpr int NBK = (\d+); \};", inplace)
    nbk = int(nbk.group(1))
    assert re.search(r"template <> struct NetGeo<DSDN> \{ static constexpr int NBK = RDN_DSDN_NBK; \};", inplace)
    assert "const int wb = 128 * nbk;" in inplace and "T = wb - 2 * H" in inplace
    assert "const int T = WB - 2 * s.halo" in cbam and "s.halo = nconv + (epi == EPI_HEAD ? 1 : 0);" in cbam
    assert "if (p16) g.T = (int)((L + g.TT - 1) / g.TT);" in cbam
    return dict(fused_halo=halo, h16_wb=const(common, "H16_WB"), wb=const(common, "WB"),
                walk_rows=macro(common, "RDN_WALK_ROWS"), walk_rows_mix=macro(common, "RDN_WALK_ROWS_MIX"),
                inplace_rows={a: 128 * (macro(inplace, "RDN_DSDN_NBK") if a == "DSDN" else nbk) for a in halo},
                team_halo=const(cbam, "TEAM_HALO"))


def test_tile_geometry_is_the_sources():
    """The seam lengths of the GPU test and the seam distances of a failure report come from
    routing_nets' geometry constants: held to the sources and to the constants the existing GPU tests
    use, so that a changed kernel geometry fails here instead of quietly moving the seams off the cases."""
    from test_forward_gpu import SHORT_TILE_HALO, _f16mix_tiles_T
    g = _source_geometry()
    assert rn.FUSED_HALO == g["fused_halo"]
    assert all(rn.FUSED_HALO[a] == h for a, h in SHORT_TILE_HALO.items())
    assert rn.PINGPONG_ROWS == g["h16_wb"] and rn.TEAM16_ROWS == g["h16_wb"] and rn.TEAM_ROWS == g["wb"]
    assert rn.WALK_T == g["walk_rows"] == g["walk_rows_mix"]
    assert rn.INPLACE_ROWS == g["inplace_rows"]
    assert rn.TEAM_HALO == g["team_halo"]
    assert rn.path_T("RRCDNet", "f16", 3001) == (_f16mix_tiles_T(3001)[0],) == (582,)
    # fp32 / f16f8 / bf16x3 run 640-row tiles everywhere but on DSDN
    assert [rn.nominal_T(a, "f16f8") for a in ("DenoiseCNN", "RRCDNet", "DSDN", "PIDN")] == [600, 582, 444, 576]
    assert [rn.nominal_T(a, "f16-short") for a in ("DenoiseCNN", "RRCDNet", "DSDN", "PIDN")] == [216, 198, 188, 192]
    # the f16 team kernel spreads L evenly over ceil(L / 628) tiles (test_forward_gpu's 500 / 628)
    assert rn.path_T("ADSDN", "fp32", 2049) == (500,) and rn.path_T("ADSDN", "f16", 1256) == (628,)
    assert rn.path_T("ADSDN", "f16", 2049) == (513,) and rn.path_T("APIDN", "f16", 1257) == (419,)
    assert rn.path_T("ADSDN", "f16", 2600, segments=True) == (512, 510, 508)
    # the extra in-place length: third tile, need = L - base + 2 = 450 rows, the 4-block body (385..512)
    for a in ("DenoiseCNN", "RRCDNet", "PIDN"):
        T, H = rn.nominal_T(a, "fp32"), rn.FUSED_HALO[a]
        L = [L for L in rn.gpu_lengths(a, "fp32") if L not in rn.gpu_lengths(a, "f16")]
        L = [x for x in L if 2 * T < x <= 3 * T and 384 < x - (2 * T - H) + 2 <= 512]
        assert L, a
    assert 2 * 600 in rn.gpu_lengths("DenoiseCNN", "bf16x3") and 2 * 582 + 1 in rn.gpu_lengths("RRCDNet", "fp32")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("arch", rn.ARCHS)
def test_chains_reach_the_last_halo_row(arch, seed):
    """y[t] depends on x[t - R] alone and on x[t + R] alone, and on neither x[t -+ (R + 1)]: R is the
    radius the fused halos are sized by."""
    R = rn.REACH[arch]
    # the CBAM networks have the conv stack of DSDN / PIDN: the same radius (their kernels exchange halos
    # per CBAM segment and have no fused_halo of their own)
    assert R == _source_geometry()["fused_halo"][{"ADSDN": "DSDN", "APIDN": "PIDN"}.get(arch, arch)]
    L, t = 2049, 1024
    x = rn.routing_inputs(seed, 1, L)
    y0 = rn.ideal_forward(arch, seed, x)["y"][0, t]
    for off, moves in ((-R, True), (R, True), (-R - 1, False), (R + 1, False)):
        x1 = x.copy()
        x1[0, t + off] += 1 / 16 if x1[0, t + off] < 1.25 else -1 / 16
        y1 = rn.ideal_forward(arch, seed, x1)["y"][0, t]
        assert (y1 != y0) == moves, (off, y0, y1)


def _perturbed(spec, key, what):
    rec = spec[key]
    cl_out = rec["chain"][0]
    cin = rec["chain_in"][0]
    if what == "tap":                                        # one router weight on the neighbouring tap
        assert rec["rows"][cl_out] == [(cin, 0, 1, 0)]
        rec["rows"][cl_out] = [(cin, 1, 1, 0)]
    elif what == "tap-right":                                # the same on the right chain
        assert rec["rows"][rec["chain"][1]] == [(rec["chain_in"][1], 2, 1, 0)]
        rec["rows"][rec["chain"][1]] = [(rec["chain_in"][1], 1, 1, 0)]
    elif what == "channels":                                 # two input channels swapped
        other = next(c for c in range(cin + 1, cin + 64) if c % 64 not in rec["chain_in"]) % 64
        swap = {cin: other, other: cin}
        rec["rows"] = [[(swap.get(ci, ci), tp, sg, k) for ci, tp, sg, k in row] for row in rec["rows"]]
    else:                                                    # one K-step (32 channels of one tap) zeroed
        ks = rn.kstep(cin, 0)
        rec["rows"] = [[e for e in row if rn.kstep(e[0], e[1]) != ks] for row in rec["rows"]]
    return spec


@pytest.mark.parametrize("what", ["tap", "tap-right", "channels", "kstep"])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("arch", rn.ARCHS)
def test_wrong_index_moves_the_output_by_a_whole_step(arch, seed, what):
    """A weight on the neighbouring tap, two swapped input channels, a zeroed K-step -- in the first,
    the middle and the last big layer -- each move the ideal y by at least 1/16 somewhere: such a bug
    cannot hide below the bar.  Behind a sigmoid head the step is taken on the head's input (the logit
    over the head's scale 2^-s, chosen so that |z| <= 4), and y itself moves by more than 100 bars."""
    x = rn.routing_inputs(seed, 2, 700)
    base = rn.ideal_forward(arch, seed, x)
    big = rn.big_layers(rn.routing_spec(arch, seed))
    for key in (big[0], big[len(big) // 2], big[-1]):
        spec = _perturbed(rn.routing_spec(arch, seed), key, what)
        r = rn.ideal_forward(arch, seed, x, spec=spec)
        dy = np.abs(r["y"] - base["y"]).max()
        if arch in rn.SIGMOID:
            s = next(v["scale"] for v in spec.values() if v["kind"] == "head")
            assert np.abs(r["logit"] - base["logit"]).max() * 2 ** s >= 1 / 16, (key, s)
            assert dy >= 100 * rn.bar(arch, base["y"], DELTA[arch]), (key, dy)
        else:
            assert dy >= 1 / 16, (key, dy)


def test_mismatch_report_names_seam_and_step():
    ideal = np.zeros((2, 1200))
    y = ideal.copy()
    assert rn.describe_mismatch(y, ideal, 0.0, 582) == ""
    y[1, 583] += 1 / 16
    y[0, 1199] = np.nan
    msg = rn.describe_mismatch(y, ideal, 0.0, (582,), "RRCDNet f16")
    assert "2 of 2400 positions" in msg
    assert "spectrum 1 position 583: p mod 582 = 1, 1 from a seam, 616 from the end" in msg
    assert "+1/16" in msg and "spectrum 0 position 1199" in msg
    msg = rn.describe_mismatch(y, ideal, 0.0, (512, 510), "segments")
    assert "p mod 512 = 71, 71 from a seam; p mod 510 = 73, 73 from a seam" in msg
