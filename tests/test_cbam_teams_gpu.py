"""The CBAM team kernels (csrc/cbam.hip team16_forward for 'f16', team_forward for fp32 / f16f8 /
bf16x3) past a team's first spectrum, against the CPU oracle.

The other oracle and golden comparisons of ADSDN / APIDN launch 1 to 6 spectra: fewer than 8 launched
teams, so one spectrum per team and no XCD-local team.  Here a team runs 2, 3 and more spectra in a
row (slot parity, tags, xmode, identity buffers and LDS rows carried over), XCD-local teams are held
to the oracle, team16 polls in 2 and 3 batches (TT >= 33), one team fills the device, and the
per-segment launches run because the spectrum needs more tiles than the device holds workgroups, not
because RDN_CBAM_SEGMENTS asks.  Every batch size is chosen with tests/cbam_teams.py (the geometry
restated) and every test asserts the regime it means to run, so another CU count fails loudly.

Bars (test_forward_gpu.py F32_REL, BF16_ABS): fp32 1e-5 * max|ref|, 16-bit 2e-2 * max(1, max|ref|);
batch independence is bitwise (slots reduced in a fixed order; XM_L2 and sc1 carry the same values).
Every forward writes into a NaN-filled output: a finite row is a written row.
"""
import numpy as np
import pytest
import torch

import cbam_teams as ct
from conftest import golden_state_dict

pytestmark = pytest.mark.gpu

ARCHS = ["ADSDN", "APIDN"]
DTYPES = ["fp32", "f16", "f16f8", "bf16x3"]
F32_REL = 1e-5
BF16_ABS = 2e-2
TEAM_WS_CONST = 256 + 4 * 256          # cbam.hip:1618 team_geo: error words + padding behind the slots and counters

_MODELS, _REFS = {}, {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _model(arch, dtype):
    import raman_mi355x as R
    if (arch, dtype) not in _MODELS:
        m = R.MODELS[arch]()
        m.load_state_dict(golden_state_dict(arch, "synth"), strict=True)
        _MODELS[arch, dtype] = m.cuda().eval().set_engine_dtype(dtype)
    return _MODELS[arch, dtype]


def _forward(arch, dtype, x_np, workspace=None):
    """engine.forward into a NaN-filled y, then the workspace's status: a hand-off timeout raises
    EngineError, a saturated e4m3 plane RangeError, and no input may have left the 16-bit modes' gate."""
    from raman_mi355x import engine
    m = _model(arch, dtype)
    x = torch.tensor(np.ascontiguousarray(x_np)).unsqueeze(1).cuda()       # a copy: the cached inputs are read-only
    y = torch.full_like(x, float("nan"))
    ws = workspace if workspace is not None else _workspace(arch, dtype, x.shape[0], x.shape[-1])
    engine.forward(arch, m.engine_code, m.packed_weights(x.device), x, out=y, check=False, workspace=ws)
    flags = ws.check()
    assert flags == 0, f"status flags {flags:#x}"
    return y.squeeze(1).cpu().numpy()


def _workspace(arch, dtype, n, L):
    from raman_mi355x import engine
    return engine.Workspace(arch, _model(arch, dtype).engine_code, n, L, torch.device("cuda", 0))


def _input(seed, n, L, spikes=()):
    """uniform(-0.2, 1.2) float32; rows `spikes` carry a 40-sample spike of +3.0, each at another
    position, held to the 16-bit modes' |x| <= 4 gate (1.2 + 3.0 would leave it)."""
    x = np.random.default_rng(seed).uniform(-0.2, 1.2, (n, L)).astype(np.float32)
    for i, r in enumerate(sorted(set(spikes))):
        if L >= 80:
            c = (97 + 389 * i) % (L - 40)
            x[r, c:c + 40] = np.minimum(x[r, c:c + 40] + 3.0, 4.0)
    return x


def _ref(arch, key, make_x):
    """(x, oracle forward of x), computed once per (arch, input) and shared by the dtypes; read-only."""
    from oracle.models import forward as oracle_forward
    if (arch, key) not in _REFS:
        x = make_x()
        ref = oracle_forward(arch, golden_state_dict(arch, "synth"), torch.tensor(x).unsqueeze(1)).squeeze(1).numpy()
        x.setflags(write=False)
        ref.setflags(write=False)
        _REFS[arch, key] = (x, ref)
    return _REFS[arch, key]


def _within_bar(y, ref, dtype, what):
    assert y.shape == ref.shape
    unwritten = np.argwhere(~np.isfinite(y).all(axis=1)).ravel()
    assert unwritten.size == 0, f"{what}: rows {unwritten[:10].tolist()} not written (or NaN)"
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(y - ref).max(axis=1)
    tol = F32_REL * scale if dtype == "fp32" else BF16_ABS * max(1.0, scale)
    print(f"{what}: {dtype} worst max-abs {err.max():.3e} at row {int(err.argmax())} (tol {tol:.3e})")
    assert err.max() <= tol, f"{what}: {dtype} row {int(err.argmax())}: {err.max():.3e} > {tol:.3e}"


def _same_bits(a, b, what):
    assert a.shape == b.shape
    assert np.isfinite(a).all() and np.isfinite(b).all(), f"{what}: a row was not written"
    bad = np.argwhere((a != b).any(axis=1)).ravel()
    assert bad.size == 0, f"{what}: rows {bad[:10].tolist()} differ, max {np.abs(a - b).max():.3e}"


def _rows(dtype, n, L):
    g = ct.team_geo(dtype, L, _cus())
    assert g.teams > 0, (dtype, L, g)
    return g, (ct.rows_team16(n, g.teams, g.TT) if dtype == "f16" else ct.rows_team(n, g.teams))


def _count(rows, team):
    return sum(1 for r in rows if r.team == team)


def _roles(rows, team):
    """the rows of a team's first, second and last spectrum"""
    mine = [i for i, r in enumerate(rows) if r.team == team]
    return [mine[0], mine[1], mine[-1]]


def _takes_team_path(ws):
    """Workspace.bytes_for(n) does not depend on n on the team path and grows with n on the segment path."""
    a, b = ws.bytes_for(1), ws.bytes_for(5)
    assert a <= b
    return a == b


# --- 1. later spectra of a team --------------------------------------------------------------------
L1 = 1300


def _subset1(dtype, n):
    """rows to re-run alone: first / second / last spectrum of a local (team16) or the first team and of
    a spread or the last team, and the batch's last row"""
    g, rows = _rows(dtype, n, L1)
    lt = ct.launched(n, g.teams)
    if dtype == "f16":
        nloc = ct.team16_nloc(lt, g.TT)
        assert nloc >= 8, f"no XCD-local team: {g}"
        assert nloc < lt, f"no spread team: {g}"
        local3 = [t for t in range(nloc) if _count(rows, t) >= 3]
        spread = [t for t in range(nloc, lt)]
        assert local3, "no local team runs 3 spectra"
        a, b = local3[len(local3) // 2], spread[-1]
        assert rows[_roles(rows, a)[0]].local and not rows[_roles(rows, b)[0]].local
    else:
        a, b = 0, lt - 1
    counts = [_count(rows, t) for t in range(lt)]
    assert min(counts) >= 2 and max(counts) >= 3, f"every team runs 2 or 3 spectra, some 3: {sorted(set(counts))}"
    assert max(r.ordinal for r in rows) >= 2
    return _roles(rows, a) + _roles(rows, b) + [n - 1]


def _batch1(arch):
    teams = ct.team_geo("f16", L1, _cus()).teams
    assert teams == ct.team_geo("fp32", L1, _cus()).teams and ct.team_geo("f16", L1, _cus()).TT == 3
    n = 2 * teams + 3
    spikes = _subset1("f16", n)[:6] + _subset1("fp32", n)[:6]
    return _ref(arch, ("later", n), lambda: _input(1300, n, L1, spikes))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("arch", ARCHS)
def test_later_spectra_of_a_team_vs_oracle(arch, dtype):
    """L = 1300: TT = 3 on both kernels (team16's middle tile runs the non-EDGE body), 85 teams on 256
    CUs, n = 2 teams + 3: every team runs 2 or 3 spectra ('f16': 80 XCD-local and 5 spread teams).
    All rows within the bar; the reversed batch (every row in another team at another ordinal), rows
    run alone, a second forward on the same workspace and one with another n give the same bits."""
    x, ref = _batch1(arch)
    n = x.shape[0]
    g, rows = _rows(dtype, n, L1)
    assert g.TT == 3 and g.teams >= 8
    sub = _subset1(dtype, n)
    ws = _workspace(arch, dtype, n, L1)
    assert _takes_team_path(ws)
    if dtype == "f16":
        assert ct.team16_teams_from_bytes(ws.bytes, TEAM_WS_CONST, g.TT) == g.teams, (ws.bytes, g)
    y = _forward(arch, dtype, x, ws)
    _within_bar(y, ref, dtype, f"{arch} L={L1} n={n}")
    _same_bits(_forward(arch, dtype, x[::-1])[::-1], y, f"{arch} {dtype} reversed batch")
    for r in sub:
        _same_bits(_forward(arch, dtype, x[r:r + 1]), y[r:r + 1],
                   f"{arch} {dtype} row {r} (team {rows[r].team}, spectrum {rows[r].ordinal}) alone")
    _same_bits(_forward(arch, dtype, x, ws), y, f"{arch} {dtype} second forward on the workspace")
    n2 = g.teams + 2
    assert ws.bytes_for(n2) <= ws.bytes and n2 < n
    _same_bits(_forward(arch, dtype, x[:n2], ws), y[:n2], f"{arch} {dtype} n={n2} on the same workspace")


# --- 2. which rows a team takes ('f16') ------------------------------------------------------------
CHUNK = 7


def _sizes2(L):
    teams = ct.team_geo("f16", L, _cus()).teams
    return {64: [7, 8, 9, teams - 1, teams, teams + 1, 2 * teams + 1],
            1300: [8, 9, teams - 1, teams, teams + 1],
            16384: [9, 10, 19]}[L]


def _chunked2(arch, L):
    """(x, the 'f16' forward of x in chunks of 7 rows): fewer than 8 launched teams, i.e. one spectrum
    per team and no XCD-local team -- the regime the oracle tests of test_forward_gpu.py hold"""
    key = (arch, "chunked", L)
    if key not in _REFS:
        g = ct.team_geo("f16", L, _cus())
        assert g.teams >= CHUNK, g
        assert all(r.ordinal == 0 and not r.local for r in ct.rows_team16(CHUNK, g.teams, g.TT))
        nmax = max(_sizes2(L))
        rows = ct.rows_team16(nmax, g.teams, g.TT)
        spikes = [0, nmax - 1] + (_roles(rows, 0) if _count(rows, 0) >= 2 else [])
        x = _input(L + 2, nmax, L, spikes)
        y = np.concatenate([_forward(arch, "f16", x[i:i + CHUNK]) for i in range(0, nmax, CHUNK)])
        assert np.isfinite(y).all()
        x.setflags(write=False)
        y.setflags(write=False)
        _REFS[key] = (x, y)
    return _REFS[key]


@pytest.mark.parametrize("L", [64, 1300, 16384])
@pytest.mark.parametrize("arch", ARCHS)
def test_team16_ranges_write_every_row(arch, L):
    """team16_forward's XCD remap, weighted team_range and launched-team count: batches around 8
    launched teams, around `teams` and past 2 teams give, row for row, the bits of the same input run
    7 rows at a time; every row written.  L = 16,384: 27 tiles, 9 teams (8 XCD-local and one spread);
    two of its rows -- a local team's later spectrum and the spread team's last -- against the oracle."""
    g = ct.team_geo("f16", L, _cus())
    assert g.teams >= 9, g
    x, y7 = _chunked2(arch, L)
    assert _takes_team_path(_workspace(arch, "f16", 1, L))
    seen_local = seen_spread = seen_later = False
    for n in _sizes2(L):
        rows = ct.rows_team16(n, g.teams, g.TT)
        seen_local |= any(r.local for r in rows)
        seen_spread |= any(not r.local for r in rows) and any(r.local for r in rows)
        seen_later |= any(r.ordinal >= 1 for r in rows)
        y = _forward(arch, "f16", x[:n])
        _same_bits(y, y7[:n], f"{arch} L={L} n={n} against chunks of {CHUNK}")
    assert seen_local and seen_later, "no XCD-local team or no second spectrum in any batch"
    if L == 16384:
        assert seen_spread and ct.team16_nloc(g.teams, g.TT) == 8 and g.teams == 9, g
        n = 19
        rows = ct.rows_team16(n, g.teams, g.TT)
        later = [i for i, r in enumerate(rows) if r.local and r.ordinal >= 1]
        assert later and not rows[n - 1].local and rows[n - 1].ordinal >= 1
        pick = [later[len(later) // 2], n - 1]
        xs, ref = _ref(arch, ("ranges", L), lambda: np.ascontiguousarray(x[pick]))
        _within_bar(_forward(arch, "f16", x[:n])[pick], ref, "f16", f"{arch} L={L} n={n} rows {pick}")


# --- 3. poll batches -------------------------------------------------------------------------------
POLL_L = {20096: (32, 1), 20097: (33, 2), 40192: (64, 2), 40193: (65, 3)}      # L: team16's (TT, poll batches)


def _batch3(arch, L):
    if L != 20097:
        return _ref(arch, ("poll", L), lambda: _input(L, 2, L, [1]))
    g = ct.team_geo("f16", L, _cus())
    n = 2 * g.teams + 1
    rows = ct.rows_team16(n, g.teams, g.TT)
    assert max(r.ordinal for r in rows) >= 2, "no team runs 3 spectra"
    first = max(range(g.teams), key=lambda t: _count(rows, t))
    return _ref(arch, ("poll", L), lambda: _input(L, n, L, _roles(rows, first) + [n - 1]))


@pytest.mark.parametrize("dtype", ["f16", "fp32", "f16f8"])
@pytest.mark.parametrize("L", sorted(POLL_L))
@pytest.mark.parametrize("arch", ARCHS)
def test_poll_batches_vs_oracle(arch, L, dtype):
    """team16 polls its team's slots 32 at a time and fetches the edge rows only in the first batch:
    TT = 32, 33, 64, 65 (one, two, two and three batches), n = 2, against the oracle; team_forward at
    the same lengths."""
    g = ct.team_geo(dtype, L, _cus())
    assert g.teams >= 2, g
    if dtype == "f16":
        assert (g.TT, ct.poll_batches(g.TT)) == POLL_L[L]
    x, ref = _batch3(arch, L)
    assert _takes_team_path(_workspace(arch, dtype, 2, L))
    _within_bar(_forward(arch, dtype, x[:2]), ref[:2], dtype, f"{arch} L={L} n=2 TT={g.TT}")


@pytest.mark.parametrize("arch", ARCHS)
def test_later_spectra_under_two_poll_batches(arch):
    """L = 20,097 (TT = 33, two poll batches), n = 2 teams + 1: a team's second and third spectrum
    under two-batch polling, all rows against the oracle."""
    L = 20097
    g = ct.team_geo("f16", L, _cus())
    assert ct.poll_batches(g.TT) == 2 and g.teams >= 2
    x, ref = _batch3(arch, L)
    assert x.shape[0] == 2 * g.teams + 1
    _within_bar(_forward(arch, "f16", x), ref, "f16", f"{arch} L={L} n={x.shape[0]} TT={g.TT}")


# --- 4. one team, and the boundary to the segments -------------------------------------------------
def _one_team_cases():
    return [("f16", "3x", 3), ("f16", "full", 2), ("f16", "over", 2), ("fp32", "full", 2), ("fp32", "over", 2),
            ("f16f8", "over", 2)]


def _length4(dtype, case):
    resident = ct.team_geo(dtype, 1, _cus()).resident
    T0 = 628 if dtype == "f16" else 500
    return {"3x": 129 * 628 + 1, "full": resident * T0, "over": resident * T0 + 1}[case]


@pytest.mark.parametrize("dtype,case,n", _one_team_cases())
@pytest.mark.parametrize("arch", ARCHS)
def test_one_team_and_the_segment_boundary(arch, dtype, case, n, monkeypatch):
    """'3x': L = 129 * 628 + 1, one team of 130 tiles runs three spectra back to back.  'full':
    TT = the resident workgroups, one team on every CU, the last shape the team path takes.  'over':
    one position more, teams == 0: the per-segment launches run without RDN_CBAM_SEGMENTS, and give
    the bits of the forced segment run.  n spectra and one alone, against the oracle."""
    L = _length4(dtype, case)
    g = ct.team_geo(dtype, L, _cus())
    ws = _workspace(arch, dtype, n, L)
    if case == "over":
        assert g.teams == 0 and g.TT == g.resident + 1, g
        assert not _takes_team_path(ws), "the team path ran"
    else:
        assert g.teams == 1, g
        assert case != "full" or g.TT == g.resident
        assert _takes_team_path(ws), "the segment path ran"
        if dtype == "f16":
            assert ct.team16_teams_from_bytes(ws.bytes, TEAM_WS_CONST, g.TT) == 1, (ws.bytes, g)
            assert [r.ordinal for r in ct.rows_team16(n, g.teams, g.TT)] == list(range(n))
    x, ref = _ref(arch, ("one", L), lambda: _input(L % 1000, n, L, [0, n - 1]))
    y = _forward(arch, dtype, x, ws)
    _within_bar(y, ref, dtype, f"{arch} L={L} n={n} TT={g.TT} teams={g.teams}")
    _within_bar(_forward(arch, dtype, x[n - 1:]), ref[n - 1:], dtype, f"{arch} L={L} n=1 (row {n - 1})")
    if case == "over":
        monkeypatch.setenv("RDN_CBAM_SEGMENTS", "1")
        y_forced = _forward(arch, dtype, x)
        monkeypatch.delenv("RDN_CBAM_SEGMENTS")
        _same_bits(y, y_forced, f"{arch} {dtype} L={L} against RDN_CBAM_SEGMENTS=1")


# --- 5. team16's own tile boundaries ---------------------------------------------------------------
TILES16 = {627: 1, 628: 1, 629: 2, 1255: 2, 1256: 2, 1257: 3, 1884: 3, 1885: 4}


@pytest.mark.parametrize("L", sorted(TILES16))
@pytest.mark.parametrize("arch", ARCHS)
def test_team16_tile_boundaries_vs_oracle(arch, L):
    """team16 tiles own up to 640 - 2*6 = 628 positions, spread evenly (T = ceil(L / TT)): lengths at
    1, 2 and 3 full tiles and one position to either side, n = 2, against the oracle (the 628-position
    counterpart of test_forward_gpu.py test_cbam_team_halo_exchange)."""
    g = ct.team_geo("f16", L, _cus())
    assert g.TT == TILES16[L] and g.T == -(-L // g.TT) and g.teams >= 2, g
    x, ref = _ref(arch, ("tiles16", L), lambda: _input(L + 11, 2, L, [1]))
    _within_bar(_forward(arch, "f16", x), ref, "f16", f"{arch} L={L} TT={g.TT} T={g.T}")
