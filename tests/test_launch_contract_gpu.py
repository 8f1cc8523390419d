"""Every launch is held to the caller's stream and to the device that holds its tensors.

The rest of the suite runs on torch's default stream of device 0, where everything is ordered anyway: a
launcher that passed 0 instead of its stream for one kernel or memset, a status reset on the wrong stream or
a hidden wait on the host would pass it.  Here each engine call runs on a side stream behind a device-side
delay (tests/launch_contract.py: the protocol and why it catches a stray null-stream operation), its outputs
are compared bit for bit with the same call on the default stream, and the stream must still be busy when
the call returns.  test_check_of_the_check runs one case the wrong way on purpose and must see the mismatch:
without it every other case could pass for the wrong reason.

The cases with tensors on a second device skip on a one-GPU machine.
"""
import functools

import pytest
import torch

from conftest import golden_state_dict, load_golden
from launch_contract import Case, calibrate, decoy, delay, on_stream, reference, run_delayed, same_bits, sentinel_

pytestmark = pytest.mark.gpu

N, L = 3, 1300                # at least two tiles of every geometry: tiles own 198 to 628 positions, 2048 and 512
DEV0 = torch.device("cuda", 0)
BINS = (20.0, 37.0, 4)
two_devices = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")


# ---- shared data: made once on device 0, copied bit for bit to another device ---------------------------
@functools.lru_cache(maxsize=None)
def _spectra0(n, length):
    """clean, noisy (n, length) fp32, the nominal SNRs and noise levels (n,), and a denoised y (median, w = 5)."""
    from raman_mi355x import engine
    with torch.cuda.device(0):
        clean, noisy, snr, nstd = engine.generate(n, 20250410, signal_length=length, device=DEV0)
        y = engine.median(noisy, 5)
        torch.cuda.synchronize()
    return {"clean": clean, "noisy": noisy, "snr": snr, "nstd": nstd, "y": y}


@functools.lru_cache(maxsize=None)
def _spectra(n, length, dev):
    d = _spectra0(n, length)
    if dev == DEV0:
        return d
    d = {k: t.to(dev) for k, t in d.items()}
    torch.cuda.synchronize(dev)
    return d


@functools.lru_cache(maxsize=None)
def _state_dict(arch):
    trained = any(k.startswith("w::") for k in load_golden(arch).files)
    return golden_state_dict(arch, "trained" if trained else "synth")


@functools.lru_cache(maxsize=None)
def _packed(arch, code, dev):
    from raman_mi355x import engine
    blob = engine.pack(arch, _state_dict(arch), code, dev)
    torch.cuda.synchronize(dev)
    return blob


def _model(arch, dtype, dev=DEV0):
    import raman_mi355x as R
    m = R.MODELS[arch]()
    m.load_state_dict(_state_dict(arch), strict=True)
    return m.to(dev).eval().set_engine_dtype(dtype)


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


# ---- the cases -------------------------------------------------------------------------------------------
def _workspace(state, arch, code, n, length, dev):
    """The stream's Workspace (made under the stream that is current at the first call), or None."""
    from raman_mi355x import engine
    if not engine.needs_workspace(arch, code):
        return None
    if "ws" not in state:
        state["ws"] = engine.Workspace(arch, code, n, length, dev)
    return state["ws"]


def _ws_clean(state):
    if "ws" in state:
        assert state["ws"].check() == 0


def forward_case(arch, dtype, dev=DEV0, n=N, length=L):
    from raman_mi355x import engine
    code = engine.resolve_dtype(arch, dtype)
    packed = _packed(arch, code, dev)
    x = _spectra(n, length, dev)["noisy"].view(n, 1, length)

    def call(ins, outs, state):
        ws = _workspace(state, arch, code, n, length, dev)
        engine.forward(arch, code, packed, ins["x"], out=outs["y"], check=False, workspace=ws)

    return Case(dev, {"x": x}, lambda: {"y": _empty((n, 1, length), torch.float32, dev)}, call, finish=_ws_clean)


def forward_metrics_case(arch, dtype, fused, dev=DEV0):
    from raman_mi355x import _lib, engine
    code = engine.resolve_dtype(arch, dtype)
    packed = _packed(arch, code, dev)
    d = _spectra(N, L, dev)

    def call(ins, outs, state):
        ws = _workspace(state, arch, code, N, L, dev)
        _, per, _, was_fused = engine.forward_metrics(arch, code, packed, ins["x"], ins["clean"], out=outs["y"],
                                                      sums=outs["sums"], per_spectrum=True, acc=outs["acc"], check=False,
                                                      workspace=ws)
        assert was_fused == fused       # the geometry the case means to run
        return {"per": per}

    outs = lambda: {"y": _empty((N, 1, L), torch.float32, dev), "sums": _empty((5,), torch.float64, dev),
                    "acc": _empty((_lib.ACC_WORDS,), torch.int64, dev)}
    return Case(dev, {"x": d["noisy"].view(N, 1, L), "clean": d["clean"]}, outs, call, zeroed=("sums", "acc"),
                unchecked=("sums",), finish=_ws_clean)


def generate_case(dev=DEV0):
    from raman_mi355x import engine
    n, length = 5, 1000

    def call(ins, outs, state):
        _, _, snr, nstd = engine.generate(n, 7, first_index=3, signal_length=length, device=dev,
                                          out=(outs["clean"], outs["noisy"]))
        return {"snr": snr, "nstd": nstd}

    return Case(dev, {}, lambda: {"clean": _empty((n, length), torch.float32, dev),
                                  "noisy": _empty((n, length), torch.float32, dev)}, call)


def metrics_case(dev=DEV0):
    from raman_mi355x import _lib, engine
    d = _spectra(N, L, dev)

    def call(ins, outs, state):
        per, _ = engine.metrics(ins["y"], ins["clean"], sums=outs["sums"], per_spectrum=True, acc=outs["acc"])
        return {"per": per}

    outs = lambda: {"sums": _empty((5,), torch.float64, dev), "acc": _empty((_lib.ACC_WORDS,), torch.int64, dev)}
    return Case(dev, {"y": d["y"], "clean": d["clean"]}, outs, call, zeroed=("sums", "acc"), unchecked=("sums",))


def _meter_ins(dev, clean_f64=False):
    d = _spectra(N, L, dev)
    clean = d["clean"].double() if clean_f64 else d["clean"]
    torch.cuda.synchronize(dev)
    return {"x": d["noisy"], "y": d["y"], "clean": clean, "key": d["snr"]}


def snr_case(clean_f64, dev=DEV0):
    from raman_mi355x import _lib, engine

    def call(ins, outs, state):
        per, _ = engine.snr(ins["x"], ins["y"], ins["clean"], key=ins["key"], bins=BINS, report=outs["report"])
        return {"per": per}

    outs = lambda: {"report": _empty((_lib.report_words(BINS[2]),), torch.int64, dev)}
    return Case(dev, _meter_ins(dev, clean_f64), outs, call, zeroed=("report",))


def physics_case(dev=DEV0):
    from raman_mi355x import _lib, engine

    def call(ins, outs, state):
        per, _ = engine.physics(ins["x"], ins["y"], ins["clean"], key=ins["key"], bins=BINS, report=outs["report"])
        return {"per": per}

    outs = lambda: {"report": _empty((_lib.phys_words(BINS[2]),), torch.int64, dev)}
    return Case(dev, _meter_ins(dev), outs, call, zeroed=("report",))


def physics_grad_case(dev=DEV0):
    from raman_mi355x import engine
    ins = _meter_ins(dev)
    del ins["key"]

    def call(ins, outs, state):
        per, _ = engine.physics_grad(ins["x"], ins["y"], ins["clean"], out=outs["grad"])
        return {"per": per}

    return Case(dev, ins, lambda: {"grad": _empty((N, L), torch.float32, dev)}, call)


def blind_case(dev=DEV0):
    from raman_mi355x import _lib, engine
    ins = _meter_ins(dev)
    del ins["clean"], ins["key"]
    bins = (0.0, 40.0, 4)

    def call(ins, outs, state):           # sigma=None: the noise estimate's own launch comes first
        per, rho, _ = engine.blind(ins["x"], ins["y"], bins=bins, report=outs["report"], rho=True)
        return {"per": per, "rho": rho}

    outs = lambda: {"report": _empty((_lib.blind_words(bins[2]),), torch.int64, dev)}
    return Case(dev, ins, outs, call, zeroed=("report",))


def fir_case(dev=DEV0):
    from raman_mi355x import engine
    w = 21
    taps = torch.hann_window(w + 2, periodic=False, dtype=torch.float64)[1:-1]
    taps = (taps / taps.sum()).to(dev)
    edge = torch.stack([torch.roll(taps, j - (w - 1) // 2) for j in range(w - 1)]).contiguous()   # (w - 1, w)
    torch.cuda.synchronize(dev)

    def call(ins, outs, state):
        engine.fir(ins["x"], ins["taps"], edge_taps=ins["edge"], out=outs["y"])

    return Case(dev, {"x": _spectra(N, L, dev)["noisy"], "taps": taps, "edge": edge},
                lambda: {"y": _empty((N, L), torch.float32, dev)}, call)


def median_case(window, dev=DEV0):
    from raman_mi355x import engine

    def call(ins, outs, state):
        engine.median(ins["x"], window, out=outs["y"])

    return Case(dev, {"x": _spectra(N, L, dev)["noisy"]}, lambda: {"y": _empty((N, L), torch.float32, dev)}, call)


def haar_case(length, dev=DEV0):
    from raman_mi355x import engine
    k = [3.0, 2.0, 1.5, 1.0]              # J = 4

    def call(ins, outs, state):
        engine.haar_shrink(ins["x"], k, mode="hard", out=outs["y"], med=outs["med"])

    return Case(dev, {"x": _spectra(N, length, dev)["noisy"]},
                lambda: {"y": _empty((N, length), torch.float32, dev), "med": _empty((N,), torch.float64, dev)}, call)


def noise_mad_case(dev=DEV0):
    from raman_mi355x import engine

    def call(ins, outs, state):
        engine.noise_mad(ins["x"], out=outs["med"])

    return Case(dev, {"x": _spectra(N, L, dev)["noisy"]}, lambda: {"med": _empty((N,), torch.float64, dev)}, call)


def potts_case(dev=DEV0):
    from raman_mi355x import engine
    gamma = torch.tensor([0.02, 0.05, 0.1], dtype=torch.float64).to(dev)
    torch.cuda.synchronize(dev)

    def call(ins, outs, state):
        engine.potts(ins["x"], ins["gamma"], out=outs["y"], nseg=outs["nseg"], work=outs["work"])

    outs = lambda: {"y": _empty((N, L), torch.float32, dev), "nseg": _empty((N,), torch.int32, dev),
                    "work": _empty((N * L,), torch.uint8, dev)}
    return Case(dev, {"x": _spectra(N, L, dev)["noisy"], "gamma": gamma}, outs, call, unchecked=("work",))


def bayes_case(dev=DEV0):
    from raman_mi355x import engine
    d = _spectra(N, L, dev)
    sigma = d["nstd"].double()
    torch.cuda.synchronize(dev)

    def call(ins, outs, state):
        engine.bayes_steps(ins["x"], ins["sigma"], out=outs["y"], jump=outs["jump"], logz=outs["logz"], work=outs["work"])

    outs = lambda: {"y": _empty((N, L), torch.float32, dev), "jump": _empty((N, L), torch.float32, dev),
                    "logz": _empty((N,), torch.float64, dev), "work": _empty((N * (L + 1),), torch.float64, dev)}
    return Case(dev, {"x": d["noisy"], "sigma": sigma}, outs, call, unchecked=("work",))


# RDN_SHORT_TILES / RDN_WALK force the forward's geometry (abi.cpp); the short tiles are tested first, so the
# walk needs them refused.  None: the switch is unset.
TILES = {"RDN_SHORT_TILES": "0", "RDN_WALK": "0"}
SHORT = {"RDN_SHORT_TILES": "1", "RDN_WALK": "0"}
WALK = {"RDN_SHORT_TILES": "0", "RDN_WALK": "1"}
TEAMS = {"RDN_CBAM_SEGMENTS": None}
SEGMENTS = {"RDN_CBAM_SEGMENTS": "1"}

# id -> (environment, factory).  No case is "synchronous by contract": every engine-level call below returned
# with its stream still busy.
CASES = {
    "forward-DenoiseCNN-f16-tiles640": (TILES, lambda: forward_case("DenoiseCNN", "f16")),
    "forward-DenoiseCNN-f16-tiles256": (SHORT, lambda: forward_case("DenoiseCNN", "f16")),
    "forward-DenoiseCNN-f16-walk": (WALK, lambda: forward_case("DenoiseCNN", "f16")),
    "forward-RRCDNet-f16-tiles640": (TILES, lambda: forward_case("RRCDNet", "f16")),
    "forward-RRCDNet-f16-walk": (WALK, lambda: forward_case("RRCDNet", "f16")),
    "forward-RRCDNet-f16f8": ({}, lambda: forward_case("RRCDNet", "f16f8")),
    "forward-RRCDNet-fp32": ({}, lambda: forward_case("RRCDNet", "fp32")),
    "forward-ADSDN-f16-teams": (TEAMS, lambda: forward_case("ADSDN", "f16")),
    "forward-ADSDN-fp32-teams": (TEAMS, lambda: forward_case("ADSDN", "fp32")),
    "forward-ADSDN-fp32-segments": (SEGMENTS, lambda: forward_case("ADSDN", "fp32")),
    "forward_metrics-RRCDNet-f16-walk": (WALK, lambda: forward_metrics_case("RRCDNet", "f16", True)),
    "forward_metrics-RRCDNet-f16-tiles640": (TILES, lambda: forward_metrics_case("RRCDNet", "f16", False)),
    "generate": ({}, generate_case),
    "metrics": ({}, metrics_case),
    "snr-fp32-clean": ({}, lambda: snr_case(False)),
    "snr-fp64-clean": ({}, lambda: snr_case(True)),
    "physics": ({}, physics_case),
    "physics_grad": ({}, physics_grad_case),
    "blind": ({}, blind_case),
    "fir-w21-edge-table": ({}, fir_case),
    "median-w5-network": ({}, lambda: median_case(5)),
    "median-w31-radix": ({}, lambda: median_case(31)),
    "haar_shrink-L1300": ({}, lambda: haar_case(1300)),
    "haar_shrink-L12289": ({}, lambda: haar_case(12289)),
    "noise_mad": ({}, noise_mad_case),
    "potts": ({}, potts_case),
    "bayes_steps": ({}, bayes_case),
}


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def test_delay_is_calibrated():
    """About 100 ms, and never below 50 ms (the calibration itself fails then)."""
    _, ms = calibrate(DEV0)
    print(f"calibrated delay: {ms:.1f} ms")
    assert ms >= 50.0


def test_check_of_the_check():
    """The wrong way on purpose: the producer of the input is delayed on a side stream and the engine call is
    issued on the default stream without waiting for it.  The call must read the decoy (valid spectra, so
    nothing can fault) and the comparison must report the mismatch: side streams here do not serialise with
    the default stream, and the delay is long enough for the cases' verdicts to mean something."""
    from raman_mi355x import engine
    x = _spectra(N, L, DEV0)["noisy"]
    other = decoy(x)
    ref = engine.median(x, 5)
    ref_decoy = engine.median(other, 5)
    staging = other.clone()
    out = sentinel_(torch.empty_like(x))
    calibrate(DEV0)
    torch.cuda.synchronize()
    assert not same_bits(ref, ref_decoy)
    s = torch.cuda.Stream(device=DEV0)
    with on_stream(s):
        delay(s)
        staging.copy_(x)
    engine.median(staging, 5, out=out)            # on the default stream: nothing orders it behind the copy
    producer_busy = not s.query()
    torch.cuda.synchronize()
    assert producer_busy
    assert not same_bits(out, ref), "the unordered call saw the delayed input: streams serialise, or the delay is too short"
    assert same_bits(out, ref_decoy)


@pytest.mark.parametrize("name", list(CASES))
def test_call_runs_on_the_callers_stream(name, monkeypatch):
    """Bit-identical to the default stream's results behind a delayed producer, and asynchronous."""
    env, factory = CASES[name]
    _setenv(monkeypatch, env)
    case = factory()
    busy, bad = run_delayed(case, reference(case))
    assert not bad, f"{name}: {bad} differ from the default stream's bits: an operation of the call ran off its stream"
    if case.waits is None:
        assert busy, f"{name}: the stream was idle when the call returned: the call waited on the host"


def test_checked_calls_wait_and_keep_their_values(monkeypatch):
    """The calls documented as waiting (check=True, Workspace.check()) are exempt from `busy`, not from the
    values: a checked forward on the side stream returns with its stream idle and the same bits."""
    from raman_mi355x import engine
    _setenv(monkeypatch, TILES)
    arch, code = "RRCDNet", engine.resolve_dtype("RRCDNet", "f16f8")
    packed = _packed(arch, code, DEV0)
    x = _spectra(N, L, DEV0)["noisy"].view(N, 1, L)

    def call(ins, outs, state):
        ws = _workspace(state, arch, code, N, L, DEV0)
        engine.forward(arch, code, packed, ins["x"], out=outs["y"], check=True, workspace=ws)

    case = Case(DEV0, {"x": x}, lambda: {"y": _empty((N, 1, L), torch.float32, DEV0)}, call, finish=_ws_clean,
                waits="check=True reads the status word behind the forward (rdn_forward_status_ex)")
    busy, bad = run_delayed(case, reference(case))
    assert not bad
    assert not busy


# ---- module level: values only ---------------------------------------------------------------------------
def _three_ways(module, x):
    """module(x) on the default stream, under a side stream, on the default stream again."""
    with torch.no_grad():
        y0 = module(x)
        torch.cuda.synchronize()
        ws0 = getattr(module, "_ws", None)
        s = torch.cuda.Stream(device=x.device)
        s.wait_stream(torch.cuda.current_stream(x.device))
        with on_stream(s):
            y1 = module(x)
            ws1 = getattr(module, "_ws", None)
        s.synchronize()
        y2 = module(x)
        ws2 = getattr(module, "_ws", None)
        torch.cuda.synchronize()
    return (y0, y1, y2), (ws0, ws1, ws2), s


def test_module_forward_follows_the_current_stream(monkeypatch):
    import raman_mi355x as R
    _setenv(monkeypatch, TILES)
    x = _spectra(N, L, DEV0)["noisy"].view(N, 1, L)
    ys, wss, s = _three_ways(_model("RRCDNet", "f16"), x)
    assert same_bits(ys[0], ys[1]) and same_bits(ys[0], ys[2]) and not torch.isnan(ys[0]).any()
    default = torch.cuda.current_stream(DEV0).cuda_stream
    # the cached workspace is bound to a stream: re-made for each
    assert [w.stream.cuda_stream for w in wss] == [default, s.cuda_stream, default]
    assert wss[0] is not wss[1] and wss[1] is not wss[2]
    ys, _, _ = _three_ways(R.MedianFilter(5), x)
    assert same_bits(ys[0], ys[1]) and same_bits(ys[0], ys[2]) and not torch.isnan(ys[0]).any()


def test_evaluate_synthetic_follows_the_current_stream(monkeypatch):
    import raman_mi355x as R
    _setenv(monkeypatch, TILES)
    models = {"cnn": _model("DenoiseCNN", "f16"), "med3": R.MedianFilter(3)}

    def run():
        return R.evaluate_synthetic(models, 64, batch_size=40, signal_length=1000, device=DEV0, snr_bins=BINS)

    r0 = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV0)
    with on_stream(s):
        r1 = run()
    s.synchronize()
    for name in models:
        assert r0[name]["acc"] == r1[name]["acc"], name            # exact accumulators: compared as words
        assert r0[name]["report"] == r1[name]["report"], name
        assert any(r0[name]["acc"]) and any(r0[name]["report"]), name


# ---- tensors and weights on a second device, the current device staying 0 ---------------------------------
DEV1_CASES = {
    "forward-DenoiseCNN-f16": (TILES, lambda dev: forward_case("DenoiseCNN", "f16", dev)),
    "forward-ADSDN-f16": (TEAMS, lambda dev: forward_case("ADSDN", "f16", dev)),
    "median-w31": ({}, lambda dev: median_case(31, dev)),
    "haar_shrink": ({}, lambda dev: haar_case(1300, dev)),
    "metrics": ({}, lambda dev: metrics_case(dev)),
}


@two_devices
@pytest.mark.parametrize("name", list(DEV1_CASES))
def test_call_runs_on_the_tensors_device(name, monkeypatch):
    """Device 0 is current, the tensors and weights live on cuda:1: the call runs there -- on cuda:1's default
    stream and, by the delayed protocol, on a side stream of it -- gives device 0's bits, and leaves device 0
    current."""
    env, factory = DEV1_CASES[name]
    _setenv(monkeypatch, env)
    dev1 = torch.device("cuda", 1)
    with torch.cuda.device(0):
        ref0 = reference(factory(DEV0))            # device 0 first: its LDS opt-ins and caches are in place
        case = factory(dev1)
        ref1 = reference(case)
        assert torch.cuda.current_device() == 0
        assert set(ref0) == set(ref1)
        for k in ref0:
            assert same_bits(ref0[k].cpu(), ref1[k].cpu()), f"{name}: {k} on cuda:1 differs from device 0's bits"
        busy, bad = run_delayed(case, ref1)
        assert torch.cuda.current_device() == 0
        assert not bad, f"{name}: {bad} differ: an operation of the call ran off its stream or its device"
        assert busy, f"{name}: the call waited on the host"
