"""The CBAM team kernels' geometry and work assignment, restated in plain Python from csrc/cbam.hip
(the precedent: _team16_place in tests/test_cpu_host.py).  tests/test_cbam_teams_gpu.py chooses its
batch sizes from these functions and asserts the regime it means to run (local teams, a team's third
spectrum, a spread team, ...), so that on a device with another CU count a test fails loudly instead
of passing on a path it did not take; tests/test_cpu_host.py checks the partition itself.

Nothing here touches the library: `cus` comes from the caller (the GPU tests pass
torch.cuda.get_device_properties(...).multi_processor_count).
"""
from collections import namedtuple

SLOT16_BYTES = 3584           # cbam.hip:928  t16::SLOT16_BYTES (448 granules of 8 B)
TEAM_CTR_BYTES = 64           # cbam.hip:341  TEAM_CTR_STRIDE u32s per team counter
POLL_STEP = 32                # cbam.hip:1136 STEP = WAVES * POLL_PER slots per poll batch
BLOCKS_PER_CU = 1             # both team kernels are LDS-bound at one workgroup per CU

Geo = namedtuple("Geo", "T TT teams resident")
Row = namedtuple("Row", "team ordinal local")


def team_geo(dtype, L, cus):
    """cbam.hip:1599-1611 team_geo: a tile owns T0 = WB - 2 * TEAM_HALO positions (640 - 12 = 628 on
    the ping-pong kernel of 'f16', 512 - 12 = 500 on team_forward), TT = ceil(L / T0) tiles make a
    team, 'f16' then spreads L evenly (T = ceil(L / TT)), and the device holds resident // TT teams
    (0: the per-segment launches run)."""
    T = 628 if dtype == "f16" else 500
    TT = -(-L // T)
    if dtype == "f16":
        T = -(-L // TT)
    resident = cus * BLOCKS_PER_CU
    return Geo(T, TT, resident // TT, resident)


def launched(n, teams):
    """cbam.hip:1676 launch_team: never more teams than spectra."""
    return min(n, teams)


def team16_nloc(teams, TT):
    """cbam.hip:1504 team16_forward: tpx one-XCD teams per XCD from the launched teams; teams
    0 .. nloc - 1 = 8 tpx - 1 are XCD-local candidates, the rest spread."""
    tpx = (teams * TT // 8) // TT
    return 8 * tpx


def poll_batches(TT):
    """cbam.hip:1137 apply16: nbatch = ceil(TT / STEP)."""
    return -(-TT // POLL_STEP)


def team_range(n, teams, team, nloc, xcd=True):
    """cbam.hip:1399-1409 team_range: [lo, hi) of `team` among `teams` launched ones.  With
    n >= teams every team takes one spectrum and the weights share out the rest, rounded up; a spread
    team weighs 31 against a local team's 32 while the XCD hand-off is on and spread teams exist.
    (The kernel only sees n >= teams, launched(); with fewer the plain weighted split, rounded up,
    gives spectrum 0 to team 0.)"""
    ws = 31 if xcd and nloc < teams else 32

    def cum(t):
        return 32 * t if t <= nloc else 32 * nloc + ws * (t - nloc)
    W = cum(teams)
    one = 1 if n >= teams else 0
    rest = n - one * teams
    lo = one * team + (rest * cum(team) + W - 1) // W
    hi = one * (team + 1) + (rest * cum(team + 1) + W - 1) // W
    return lo, hi


def rows_team16(n, teams, TT, xcd=True):
    """Per row of an 'f16' launch of n spectra on a device that holds `teams` teams of TT tiles:
    Row(team, ordinal within the team, team is an XCD-local candidate)."""
    lt = launched(n, teams)
    nloc = team16_nloc(lt, TT)
    out = [None] * n
    for t in range(lt):
        lo, hi = team_range(n, lt, t, nloc, xcd)
        for r in range(lo, hi):
            assert out[r] is None, (r, t)
            out[r] = Row(t, r - lo, t < nloc)
    return out


def rows_team(n, teams):
    """cbam.hip:803 team_forward: `for (n = team; n < ta.n; n += ta.teams)` -- row r is the
    (r // teams)-th spectrum of team r % teams (no XCD-local teams on this kernel)."""
    lt = launched(n, teams)
    return [Row(r % lt, r // lt, False) for r in range(n)]


def team16_teams_from_bytes(nbytes, const, TT):
    """cbam.hip:1615-1618 team_geo: the 'f16' team-path workspace is
    teams * (2 TT SLOT16_BYTES + TEAM_CTR_BYTES) + const (no identity buffers); returns teams, or None
    if that does not divide out."""
    per = 2 * TT * SLOT16_BYTES + TEAM_CTR_BYTES
    q, r = divmod(nbytes - const, per)
    return q if r == 0 and q > 0 else None
