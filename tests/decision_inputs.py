"""Inputs for the decision stage (rtabmap_amd/csrc/bayes.hip) at the sizes where its launch plan and its neighbour lists change shape.
Every generator states a property; tests/test_decision_inputs.py proves it without a GPU.  A generator whose property fails for a seed
takes the next seed, MAX_SEEDS at the most (asserted)."""
import numpy as np

from bayes_model import DEFAULT_LC, Graph
from decision_model import Statistics, chain_depth, f32

# ---- read from rtabmap_amd/csrc/bayes.hip: a change there is one edit here
DC_BLOCK = 256                      # constexpr int DC_BLOCK: threads per workgroup of the passes
SLOTS_PLAIN = DC_BLOCK              # SPB = DC_BLOCK / LPS with LPS = 1: slots per workgroup step, likelihood statistics alone
SLOTS_BAYES = DC_BLOCK // 8         # LPS = 8: eight lanes walk a slot's neighbour list
DC_MAX_GRID = 1024                  # constexpr int DC_MAX_GRID: workgroups per pass at the most, then the grid-stride loop makes more trips
FOLD_PROLOGUE = DC_BLOCK            # fold1<DC_BLOCK> in pass 2's prologue: more partials than this take the PER branch
DC_FOLD = 1024                      # decide_fold1_kernel / decide_fold2_kernel: one workgroup of 16 waves
ROWS = 6                            # list rows of 8 entries requested per round trip
ROUND_TRIP = ROWS * 8               # 48 entries
K_INITIAL = 64                      # Bayes::K before any list outgrows it (bayes.h); doubles: 64 -> 128 -> 256
CAP_INITIAL = 4096                  # Bayes::ensure: ncap = cap ? cap : 4096, doubles
DEPTH = DEFAULT_LC.shape[0] - 1     # Memory::getNeighborsId's depth for the default pattern: a chain neighbourhood is 2 * (DEPTH - 1) + 1 entries
CHAIN_LIST = 2 * (DEPTH - 1) + 1    # 33
MAX_SEEDS = 8


def launch_plan(n_slots, bayes=False):
    """Bayes::decide's grid for n_slots, the trips of the grid-stride loop, the fold's PER and the longest chain of additions."""
    spb = SLOTS_BAYES if bayes else SLOTS_PLAIN
    grid = int(min(DC_MAX_GRID, max(1, -(-n_slots // spb))))
    stride = grid * spb
    trips = max(1, -(-n_slots // stride))
    per = DC_MAX_GRID // FOLD_PROLOGUE if grid > FOLD_PROLOGUE else 0
    # either fold may run (decide_fold1_kernel without d_adjusted: 16 waves, never PER; pass 2's prologue: 4 waves): the longer chain
    chain = max(chain_depth(trips, 0, DC_FOLD // 64), chain_depth(trips, per, FOLD_PROLOGUE // 64))
    return dict(spb=spb, grid=grid, stride=stride, trips=trips, per=per, chain=chain)


def named_slots(n_slots, bayes=False):
    """Where a maximum is worth placing: the first slot, the last, the first slot of the last workgroup's last step, the last slot the
    second grid-stride trip serves (when there is one)."""
    p = launch_plan(n_slots, bayes)
    out = {"first": 0, "last": n_slots - 1, "last_workgroup": ((n_slots - 1) // p["spb"]) * p["spb"]}
    if p["trips"] >= 2:
        out["second_trip"] = min(n_slots, 2 * p["stride"]) - 1
    return out


def statistics(L, considered=None, mean=None):
    L = np.asarray(L)
    return Statistics(L, considered, chain=launch_plan(max(L.shape[0], 1))["chain"], mean=mean)


def all_decided(L):
    st = statistics(L)
    return all(st.adjust(r).decided.all() for r in (0.0, 0.5))


def _seeded(make, ok, seed):
    for k in range(MAX_SEEDS):
        v = make(seed + k)
        if ok(v):
            return v, k
    raise AssertionError("no seed in %d..%d gives the property" % (seed, seed + MAX_SEEDS - 1))


def stat_vector(n_slots, max_at, seed=0, with_seed=False):
    """About 70 % positive log-normal values (stddev / mean about 1), zeros elsewhere, the maximum at slot `max_at`.
    Property: no entry is undecided at either ratio."""
    def make(s):
        rng = np.random.default_rng(s)
        L = np.exp(rng.normal(-3.0, 0.8, n_slots)).astype(f32)
        L[rng.random(n_slots) >= 0.7] = 0
        L[max_at] = f32(1.5) * max(L.max(), f32(0.05))
        return L
    v, k = _seeded(make, all_decided, 1000 * seed)
    return (v, k) if with_seed else v


def exact_vector(n_slots, m=8, d=4, raised=False, seed=0):
    """c entries m - d, c entries m + d and one entry m, small integers, at least one in every workgroup step (c = the fewest that reach
    every step), zeros elsewhere: every sum is an exact integer in double, mean = m, var = d^2, stddev = d.  The top entries EQUAL the
    threshold m + d: every adjusted entry is 1.0, L[0] = m / d + 1 (ratio 0) or d / d + 1 = 2 (ratio != 0), bit for bit.
    raised: the c top entries one float ulp higher.  In exact arithmetic that lifts the threshold by (1 - 1 / (4 c + 2)) ulp -- the mean by
    c / (2 c + 1) ulp, the deviation by half an ulp -- so whether they are selected is decided by float rounding behind the statistics,
    and the model's bounds (1.5 ulp on stddev) leave them undecided.  Properties: the mean is decided (it rounds back to m whatever the
    sum's error) and so is the float the variance is converted to; with a correctly rounded sqrtf the device then makes the model's own
    float32 operations: mean m, stddev the float above d, threshold m + d by round-to-even, the raised entries selected, the rest not.
    Returns (vector, c)."""
    steps = -(-n_slots // SLOTS_PLAIN)
    c = min(steps + 1, (n_slots - 1) // 2)                             # 2 c + 1 > 2 * steps: jittered positions are less than a step apart
    rng = np.random.default_rng(seed)
    k = 2 * c + 1
    pos = (np.arange(k) * n_slots) // k                               # strictly increasing while k <= n_slots; a gap is at most a step
    pos = np.minimum(pos + rng.integers(0, max(n_slots // k, 1), k), n_slots - 1) if n_slots >= 2 * k else pos
    pos[-1] = n_slots - 1                                             # the last step may hold a single slot
    pos = np.unique(pos)
    assert pos.shape[0] == k
    vals = np.concatenate([np.full(c, m - d), np.full(c, m + d), [m]]).astype(f32)
    if raised:
        vals[c:2 * c] = np.nextafter(f32(m + d), f32(np.inf))
    L = np.zeros(n_slots, f32)
    L[pos] = vals[rng.permutation(k)]
    return L, c


def sparse_vector(n_slots, kind, seed=0):
    """one: exactly one positive entry (CP = 1, variance 0);  two: exactly two equal ones;  none: no positive entry (the result is
    [2, 1, 1, ...]);  last_partial: positives only in slots the LAST partial of the fold covers (the last workgroup of the grid)."""
    rng = np.random.default_rng(seed)
    L = np.zeros(n_slots, f32)
    if kind == "one":
        L[int(rng.integers(0, n_slots))] = f32(0.37)
    elif kind == "two":
        L[rng.choice(n_slots, size=min(2, n_slots), replace=False)] = f32(0.37)
    elif kind == "last_partial":
        p = launch_plan(n_slots)
        s = np.arange(n_slots)
        mine = s[(s // p["spb"]) % p["grid"] == p["grid"] - 1]
        pick = rng.choice(mine, size=min(12, mine.shape[0]), replace=False)
        L[pick] = np.exp(rng.normal(-3.0, 0.8, pick.shape[0])).astype(f32)
        L[pick[0]] = f32(1.0)
    else:
        assert kind == "none"
    return L


def near_cancel_vector(n_slots, seed=0):
    """About 70 % of the entries 1 +- 1e-4: S2 - 2 m S1 + CP m^2 cancels eight digits.  Property: the model's own bound on stddev stays
    below 1e-3 relative, so a test can still assert something -- within that bound."""
    def make(s):
        rng = np.random.default_rng(s)
        L = (1.0 + 1e-4 * rng.choice([-1.0, 1.0], n_slots)).astype(f32)
        L[rng.random(n_slots) >= 0.7] = 0
        return L

    def ok(L):
        st = statistics(L)
        return st.n_positive < 2 or (st.stddev > 0 and st.std_tol < 1e-3 * float(st.stddev))
    return _seeded(make, ok, 1000 * seed + 500)[0]


# ---- graphs: an odometry chain plus loop links placed so that the neighbour lists have the lengths the list walk changes shape at
# a loop link a <-> a - g with g <= 2 * (DEPTH - 1) joins two overlapping neighbourhoods: both ends list CHAIN_LIST + g signatures;
# a second link from a to a far place adds that place's CHAIN_LIST
BOUNDARY_LENGTHS = (47, 48, 49, 64, 65, 96, 97)
SPACING = 120


def boundary_graph(n, extra_loops=()):
    """Returns (graph, info).  info: `anchors` {list length: signature id with that length}, `stm` (how many of the newest signatures a test
    should exclude so that a list above 48 entries reaches into the short-term memory), `retire` (ids to retire: neighbours of long lists and
    a few around workgroup boundaries).  A structure that does not fit below n is left out: all seven fit from n = 1100."""
    loops, anchors = [], {}
    base = 100
    for length in BOUNDARY_LENGTHS:
        g = length - CHAIN_LIST if length < 2 * CHAIN_LIST else length - 2 * CHAIN_LIST
        a = base + g
        far = a + 60
        top = far + DEPTH if length >= 2 * CHAIN_LIST else a + DEPTH
        if top < n - 80:
            loops.append((a, base))
            if length >= 2 * CHAIN_LIST:
                loops.append((a, far))
            anchors[length] = a
        base += SPACING
    stm = 30
    if n >= 260:                                   # a list of 65 whose upper end lies in the short-term memory, its anchor below it
        a = n - stm - 8
        loops.append((a, a - 32))
        anchors["stm"] = a
    elif n >= 20:
        loops.append((n - 2, 3))
    retire = sorted(set([a - 3 for a in anchors.values()] + [s for s in (SLOTS_BAYES, SLOTS_BAYES + 1, 8 * SLOTS_BAYES, 8 * SLOTS_BAYES + 2) if s < n - stm - 60]))
    return Graph(n, loops + list(extra_loops)), dict(anchors=anchors, stm=stm, retire=retire)


def hub_graph(n):
    """One signature with four loop links to places more than 40 apart: its list and those of the four places hold 5 * CHAIN_LIST = 165
    entries, past 128, so the table's width K doubles twice.  Returns (graph, hub id, the four places)."""
    places = [100, 200, 300, 400]
    hub = 550
    assert n >= hub + 60
    return Graph(n, [(hub, p) for p in places]), hub, places


def list_lengths(off):
    return np.diff(np.asarray(off))
