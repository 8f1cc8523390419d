"""Every engine path against the exact-arithmetic routing networks (tests/routing_nets.py).

The weights are +-2^k routers, the inputs k/16, BatchNorm the identity up to its fold residue and every
CBAM exactly 1/4, so one f16 MFMA per product, the f16 + e4m3 corrected product, the three split-bf16
products and the compensated fp32 chain all return the same exact number: the kernels must reproduce an
integer evaluation of the network (routing_nets.ideal_forward; never another engine path), and a
mis-indexed row, tap, channel, layer, halo or hand-off is a discrete error of at least one input step
(1/16) instead of something inside the 2e-2 product bar of test_forward_gpu.py.

Bars (routing_nets.bar): 1DCNN bitwise equal in every mode; RRCDNet / DSDN / ADSDN 2 delta + 2^-23 max(1,
max|ideal|); PIDN / APIDN 2 delta + 4 * 2^-24 against the float64 sigmoid of the exact logit (the engine
does not expose its logit); delta = the BatchNorm fold's residue measured in test_routing_cpu.py.

Two device facts the exactness of these cases rests on, measured on an MI355X by this file:
  * the f16 team kernel's sigmoid (cbam.hip sigm_fast: v_exp_f32 + v_rcp_f32, rounded to f16) of 0 is
    exactly 1/2: ADSDN / APIDN 'f16' land on the ideal, which they could not with any other factor;
  * an all-zero e4m3 block (both lo planes of f16f8 are zero here, in every layer) contributes an exact
    zero through the packer and the block-scaled MFMA: 'f16f8' lands on the ideal on all six networks.
"""
import functools

import numpy as np
import pytest
import torch

import routing_nets as rn
from test_routing_cpu import DELTA          # the BatchNorm fold's residue, measured there

pytestmark = pytest.mark.gpu

N = 3                                   # spectra per call
CASES = [(a, m) for a in rn.ARCHS for m in rn.modes(a)]


@functools.lru_cache(maxsize=None)
def _inputs_and_ideal(arch, seed, L, spiked_rows=()):
    """(x, ideal y), computed once and shared by every mode; read-only."""
    x = rn.spiked_inputs(seed, N, L, rows=spiked_rows) if spiked_rows else rn.routing_inputs(seed, N, L)
    y = rn.ideal_forward(arch, seed, x)["y"]
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _tiles(mode, monkeypatch):
    """test_forward_gpu._tiles: 'f16' on the 640-row tiles, 'f16-short' on the 256-row tiles, '-walk' on
    the walk geometry (RDN_SHORT_TILES / RDN_WALK force the geometry); returns the module dtype."""
    if mode in ("f16", "f16-plain", "f16-short", "f16-walk", "f16-plain-walk"):
        monkeypatch.setenv("RDN_SHORT_TILES", "1" if mode == "f16-short" else "0")
        monkeypatch.setenv("RDN_WALK", "1" if mode.endswith("walk") else "0")
        return "f16-plain" if mode.startswith("f16-plain") else "f16"
    return mode


def _model(arch, seed, dtype):
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(rn.routing_state_dict(arch, seed), strict=True)
    return m.cuda().eval().set_engine_dtype(dtype)


def _run(m, x_np):
    x = torch.from_numpy(np.array(x_np, dtype=np.float32)).unsqueeze(1).cuda()     # a writable copy
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.dtype == torch.float32
    return y.squeeze(1).cpu().numpy()


def _bar(arch, ideal):
    return rn.bar(arch, ideal, DELTA[arch])


def _verdict(arch, mode, m, seed, L, spiked_rows=(), segments=False):
    """('' or the mismatch report, max error) of one launch against the ideal."""
    x, ideal = _inputs_and_ideal(arch, seed, L, spiked_rows)
    y = _run(m, x)
    what = f"{arch} {mode} seed {seed}" + (f" spiked {list(spiked_rows)}" if spiked_rows else "")
    msg = rn.describe_mismatch(y, ideal, _bar(arch, ideal), rn.path_T(arch, mode, L, segments), what)
    if arch == "DenoiseCNN" and not msg:
        assert np.array_equal(y, ideal)
    err = float(np.abs(y - ideal).max()) if np.isfinite(y).all() else float("nan")
    return msg, err


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("arch,mode", CASES)
def test_routing_network_is_exact(arch, mode, seed, monkeypatch):
    """One pack, then one launch per length (routing_nets.gpu_lengths: 1, 2, 5, R, R + 1, 2R + 1, 2049,
    3001, 2T and 2T + 1 for the tile this path really runs, and on the 640-row in-place kernels one
    length whose last tile takes the 4-block body; seed 2 at 2049 only)."""
    m = _model(arch, seed, _tiles(mode, monkeypatch))
    failures, worst = [], 0.0
    for L in (rn.gpu_lengths(arch, mode) if seed < 2 else [2049]):
        msg, err = _verdict(arch, mode, m, seed, L)
        worst = max(worst, err) if err == err else err
        if msg:
            failures.append(msg)
    print(f"routing {arch} {mode} seed {seed}: max |y - ideal| = {worst:.3e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", ["f16", "f16-short", "f16-walk"])
def test_routing_rrcdnet_hybrid_spiked_spectrum(mode, monkeypatch):
    """RRCDNet 'f16' with spikes (up to 2.0: outside the window [-0.3, 1.3], below the gate) in one
    spectrum of three: its spiked tiles run all-corrected, its neighbours the hybrid; both exact."""
    m = _model("RRCDNet", 0, _tiles(mode, monkeypatch))
    msg, err = _verdict("RRCDNet", mode, m, 0, 3001, spiked_rows=(1,))
    print(f"routing RRCDNet {mode} spiked: max |y - ideal| = {err:.3e}")
    assert not msg, msg


@pytest.mark.parametrize("arch", rn.ARCHS)
def test_routing_f16f8_spiked(arch):
    m = _model(arch, 0, "f16f8")
    msg, err = _verdict(arch, "f16f8", m, 0, 2049, spiked_rows=(0, 2))
    print(f"routing {arch} f16f8 spiked: max |y - ideal| = {err:.3e}")
    assert not msg, msg


@pytest.mark.parametrize("dtype", ["fp32", "f16"])
@pytest.mark.parametrize("arch", rn.CBAM)
def test_routing_cbam_segment_path(arch, dtype, monkeypatch):
    """The per-segment launches (RDN_CBAM_SEGMENTS=1, the fallback for spectra longer than the team
    geometry) on several tiles."""
    monkeypatch.setenv("RDN_CBAM_SEGMENTS", "1")
    m = _model(arch, 0, _tiles(dtype, monkeypatch))
    msg, err = _verdict(arch, dtype, m, 0, 2600, segments=True)
    print(f"routing {arch} {dtype} segments: max |y - ideal| = {err:.3e}")
    assert not msg, msg


def test_routing_report_catches_a_moved_tap(monkeypatch):
    """The check itself: RRCDNet 'f16' loaded with the routing weights but one weight of the last big
    layer (the left chain's, left_net.18.0) moved to the neighbouring tap.  Against the unperturbed ideal
    the report must name wrong positions in whole input steps; against the ideal of the perturbed network
    the engine is exact again."""
    from conftest import golden_template, load_golden
    arch, seed, L = "RRCDNet", 0, 2049
    spec = rn.routing_spec(arch, seed)
    key = rn.big_layers(spec)[-1]
    rec = spec[key]
    (cin, tap, sign, k), = rec["rows"][rec["chain"][0]]
    rec["rows"][rec["chain"][0]] = [(cin, 1, sign, k)]
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(rn.spec_state_dict(spec, golden_template(load_golden(arch))), strict=True)
    m = m.cuda().eval().set_engine_dtype(_tiles("f16", monkeypatch))
    x, ideal = _inputs_and_ideal(arch, seed, L)
    y = _run(m, x)
    msg = rn.describe_mismatch(y, ideal, _bar(arch, ideal), rn.path_T(arch, "f16", L), "moved tap")
    print(msg)
    wrong = int((np.abs(y - ideal) > _bar(arch, ideal)).sum())
    assert wrong > N * L // 2 and f"{wrong} of {N * L} positions" in msg and "/16" in msg
    assert np.abs(y - ideal).max() >= 1 / 16
    moved = rn.ideal_forward(arch, seed, x, spec=spec)["y"]
    assert rn.describe_mismatch(y, moved, _bar(arch, moved), rn.path_T(arch, "f16", L)) == ""
