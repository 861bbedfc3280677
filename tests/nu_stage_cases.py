"""The cases of tests/test_gpu_nu_stages.py and tests/test_nu_stage_model_cpu.py: small read sets from fixed seeds (low
thousands of reads at most), each with the exception list already laid out as the producers would -- groups of 128 slots
and the overflow region -- so that a case can shape the layout.  CASES maps a name to a builder, GIVE_UP the give-up cases
to what each ends on; what the MODEL must show on a case (the edge it is there for) is checked on the CPU
(tests/test_nu_stage_model_cpu.py: EXPECT).

A case: lengths, roff, starts / ends (contig-local, the reads of contig c at [roff[c], roff[c + 1])), ell, M, form
("ev" | "gen" | "gen_cuts"), rounds_max, suspects_cap, and from lay_out(): boff, cnt, slots, over (rows of global
start, global end, read index)."""
import numpy as np

GROUP = 128
DEFAULT_FILL = (96, 128, 0, 1, 127, 64, 128, 128)     # filled slots of the first groups; what is left goes to the overflow region
MAX_GROUPS = 8                                        # (the smallest list the product sizes has eight groups)


class Reads:
    def __init__(self, lengths):
        self.lengths = [int(v) for v in lengths]
        self.per = [[] for _ in self.lengths]

    def add(self, c, s, e, count=1):
        assert 0 <= s <= e < self.lengths[c], (c, s, e)
        self.per[c] += [(int(s), int(e))] * count
        return self

    def random(self, c, seed, ell, M, depth, frac, max_clip, lo=0, hi=None, frac_from=0):
        """reads of span ell at `depth` x M over [lo, hi) of contig c; a share `frac` of those starting at or behind
        frac_from is clipped by 1 .. max_clip positions at either end"""
        hi = self.lengths[c] if hi is None else hi
        rng = np.random.default_rng(seed)
        n = int(depth * M * (hi - lo) / ell)
        s = rng.integers(lo, hi - ell + 1, size=n)
        e = s + ell - 1
        pick = (rng.random(n) < frac) & (s >= frac_from)
        clip = rng.integers(1, max_clip + 1, size=n)
        front = rng.random(n) < 0.5
        s2 = np.where(pick & front, s + clip, s)
        e2 = np.where(pick & ~front, e - clip, e)
        for a, b in zip(s2, e2):
            self.add(c, a, b)
        return self

    def arrays(self):
        s, e, counts = [], [], []
        for reads in self.per:
            reads = sorted(reads, key=lambda r: r[0])
            s += [r[0] for r in reads]
            e += [r[1] for r in reads]
            counts.append(len(reads))
        return np.array(s, np.int64), np.array(e, np.int64), np.array(counts, np.int64)


def lay_out(case, fill=DEFAULT_FILL, order_seed=None):
    """the exceptions into groups of `fill` filled slots, the rest into the overflow region"""
    ell = case["ell"]
    poff = np.concatenate([[0], np.cumsum(case["lengths"])])
    contig = np.repeat(np.arange(len(case["lengths"])), np.diff(case["roff"]))
    gs = case["starts"] + poff[contig]
    ge = case["ends"] + poff[contig]
    span = ge - gs + 1
    assert (span <= ell).all() and (span >= 1).all()
    regular = span == ell
    ltot = int(poff[-1])
    case["boff"] = np.concatenate([[0], np.cumsum(np.bincount(gs[regular], minlength=ltot)[:ltot])]).astype(np.int64)
    exc = np.flatnonzero(~regular)
    if order_seed is not None:
        exc = np.random.default_rng(order_seed).permutation(exc)
    rows = np.stack([gs[exc], ge[exc], exc], axis=1).astype(np.int64).reshape(-1, 3)
    cnt, at = [], 0
    for k in fill[:MAX_GROUPS]:
        k = min(k, rows.shape[0] - at)
        cnt.append(k)
        at += k
    case["cnt"] = np.array(cnt, np.int64)
    case["slots"], case["over"] = rows[:at], rows[at:]
    case["gs"], case["ge"], case["regular"] = gs, ge, regular
    return case


def make_case(name, reads, ell, M, form, rounds_max=40, suspects_cap=4096, fill=DEFAULT_FILL, order_seed=None):
    s, e, counts = reads.arrays()
    case = {"name": name, "lengths": np.array(reads.lengths, np.int64), "roff": np.concatenate([[0], np.cumsum(counts)]),
            "starts": s, "ends": e, "n": int(s.size), "ell": int(ell), "M": int(M), "form": form, "rounds_max": int(rounds_max),
            "suspects_cap": int(suspects_cap)}
    return lay_out(case, fill, order_seed)


# ------------------------------------------------------------------------------------------------------------ builders
def spans(ell, form, M=None, seed=0):
    """one contig of some 40 spans at 3 x M with 8 % of the reads clipped (a large M: 24 spans at 1.6 x M)"""
    M = M if M is not None else (3 if ell < 32 else 6)
    L = (max(40 * ell, 300) if M < 50 else 24 * ell) + 7
    depth = 4.0 if M == 1 else 3.0 if M < 50 else 1.6
    r = Reads([L]).random(0, 100 + seed + ell, ell, M, depth, 0.08, ell - 1)
    return make_case("span%d_%s_M%d" % (ell, form, M), r, ell, M, form)


def many_rounds(form, ell, M, L, depth, frac, seed):
    r = Reads([L]).random(0, seed, ell, M, depth, frac, ell - 1)
    return make_case("rounds_%s_%d" % (form, ell), r, ell, M, form, rounds_max=60)


def contigs(form):
    """three contigs with an empty one between, then one shorter than the span that holds exceptions only, deeper than
    M; buckets before position 0 and in the previous contig; exceptions at a contig's first and last position and one
    ending at the axis' last position"""
    ell, M = 32, 3
    r = Reads([420, 0, 20, 333])
    r.random(0, 11, ell, M, 3.0, 0.1, 31).random(3, 12, ell, M, 3.0, 0.1, 31)
    r.add(0, 0, 9).add(0, 2, 25).add(0, 0, 30)             # buckets at -22, -6, -1
    r.add(0, 400, 419).add(0, 419, 419)                      # ... at a contig's last position
    for k in range(7):                                       # the short contig: exceptions only, 7 deep > M
        r.add(2, k % 3, 19 - (k % 2))
    r.add(2, 0, 0)
    r.add(3, 0, 12).add(3, 5, 20)                            # buckets in the short contig / the one before
    r.add(3, 310, 332).add(3, 332, 332)                      # ending at ltot - 1
    return make_case("contigs_%s" % form, r, ell, M, form)


def layout(which):
    """one read set, three layouts: no overflow entries (groups of 0, 1, 127, 128), one, a few hundred"""
    ell, M = 33, 5
    r = Reads([4000]).random(0, 21, ell, M, 3.0, 0.3, 32)
    n_exc = int((r.arrays()[1] - r.arrays()[0] + 1 != ell).sum())
    fills = {"over0": (0, 1, 127, 128, 128, 128, 128, 128), "over1": None, "over_many": (0, 1, 127, 128, 5, 0, 0, 0)}
    fill = fills[which]
    if which == "over1":
        rest = n_exc - 1 - (1 + 127 + 128)
        assert 0 < rest <= 4 * 128
        fill = (0, 1, 127, 128) + tuple(min(128, max(0, rest - 128 * k)) for k in range(4))
    case = make_case("layout_%s" % which, r, ell, M, "ev", fill=fill, order_seed=5)
    assert case["over"].shape[0] == {"over0": 0, "over1": 1}.get(which, case["over"].shape[0])
    assert which != "over_many" or case["over"].shape[0] >= 200
    return case


def ties():
    """nine exceptions with one start and end on an empty stretch, M = 4: the four smallest read indices are wanted at
    the same time (from a cut point: nothing but used-up buckets below them); twice, the second lot with other reads around"""
    ell, M = 64, 4
    r = Reads([3000]).random(0, 31, ell, M, 3.0, 0.05, 63, lo=0, hi=1800)
    r.add(0, 2100, 2140, count=9)
    r.add(0, 900, 940, count=9)
    return make_case("ties", r, ell, M, "gen")


def prepick():
    """an exception that starts where cov_all is exactly M (selected on release) and one where it is M + 1 (not)"""
    ell, M = 32, 4
    r = Reads([700]).random(0, 41, ell, M, 3.0, 0.05, 31, lo=300, hi=700)
    r.add(0, 100, 131, count=3).add(0, 103, 120)             # cov_all(103) = 4
    r.add(0, 200, 231, count=4).add(0, 203, 220)             # cov_all(203) = 5
    return make_case("prepick", r, ell, M, "ev")


def _exact_cover(r, c, lo, hi, ell, M, step_exc=40):
    """regular reads that cover [lo + ell, hi) exactly M deep (one every ell / M positions: every bucket is used up) under
    exceptions of ell - 1 positions that leave no cut point"""
    assert ell % M == 0
    for p in range(lo, hi - ell + 1, ell // M):
        r.add(c, p, p + ell - 1)
    for p in range(lo + 1, hi - ell, step_exc):
        r.add(c, p, p + ell - 2)


def reach(which):
    ell, M = 64, 4
    if which == "far":
        # an anchor (a pile of ten at 200), then used-up buckets for five spans: exceptions from the second span on go
        # through the far list; a missing regular read at three spans makes one of them wanted
        r = Reads([900])
        r.add(0, 200, 263, count=10)
        _exact_cover(r, 0, 216, 600, ell, M)
        r.per[0].remove((216 + 12 * 16, 216 + 12 * 16 + 63))
        r.random(0, 51, ell, M, 3.0, 0.0, 1, lo=620, hi=900)
    elif which == "cut":
        # an anchor, four spans of used-up buckets, one position without an exception over it (a cut point), five more spans
        r = Reads([1100])
        r.add(0, 100, 163, count=10)
        _exact_cover(r, 0, 116, 116 + 4 * 64, ell, M)
        q = 116 + 4 * 64
        for p in range(116 + 4 * 64 - 48, q + 5 * 64, 16):
            if (p, p + 63) not in r.per[0]:
                r.add(0, p, p + 63)
        for p in range(q + 1, q + 5 * 64, 40):
            r.add(0, p, p + 62)
        r.per[0] = [x for x in r.per[0] if not (x[1] - x[0] == 62 and x[0] <= q <= x[1])]
    elif which == "none":
        # nine spans of used-up buckets from the contig's start on, no cut point behind the first span: the exceptions
        # beyond six spans have neither an anchor nor a cut point, and nothing earlier is open
        r = Reads([800])
        _exact_cover(r, 0, 0, 760, ell, M)
    else:
        # the same run behind an empty stretch with nine exceptions of one start and end, four of them wanted at 50: in
        # round 1 the unresolved keys are not the contig's earliest and the rounds go on; in round 2 nothing those
        # exceptions read has changed (no dirty cell), and they are replayed all the same because of the key they kept
        r = Reads([1300])
        r.add(0, 50, 90, count=9)
        _exact_cover(r, 0, 300, 300 + 760, ell, M)
    return make_case("reach_%s" % which, r, ell, M, "gen", rounds_max=12)


def limit_others():
    """1 100 exceptions selected on release over one stretch: each has more than 1 024 selected neighbours (flag 4)"""
    ell, M = 64, 2000
    r = Reads([400]).add(0, 100, 163, count=40)
    for k in range(1100):
        r.add(0, 110 + k % 5, 150 + k % 7)
    return make_case("limit_others", r, ell, M, "gen", rounds_max=3)


def limit_suspects():
    """a suspects list of 64 entries and 90 selected exceptions (flag 2: nothing is written past any list)"""
    ell, M = 32, 200
    r = Reads([600]).random(0, 61, ell, 5, 3.0, 0.0, 1)
    for k in range(90):
        r.add(0, 6 * k, 6 * k + 20)
    return make_case("limit_suspects", r, ell, M, "ev", rounds_max=3, suspects_cap=64)


def restart_ev():
    """210 blocks of 32 positions; clipped reads only beyond block 135: the second chain restarts at block 128"""
    ell, M = 32, 4
    L = 210 * 32
    r = Reads([L]).random(0, 71, ell, M, 3.0, 0.25, 31, frac_from=136 * 32)
    return make_case("restart_ev", r, ell, M, "ev")


def restart_cuts():
    """two contigs, 5 windows of 64 blocks: gaps give real cut points, clipped reads in only some stretches"""
    ell, M = 32, 3
    r = Reads([6200, 4040])
    r.random(0, 81, ell, M, 2.5, 0.0, 1, lo=0, hi=1500)
    r.random(0, 82, ell, M, 2.5, 0.25, 31, lo=1540, hi=3100)
    r.random(0, 83, ell, M, 2.5, 0.0, 1, lo=3150, hi=4700)
    r.random(0, 84, ell, M, 2.5, 0.2, 31, lo=4700, hi=6200)
    r.random(1, 85, ell, M, 2.5, 0.0, 1, lo=0, hi=2000)
    r.random(1, 86, ell, M, 2.5, 0.25, 31, lo=2100, hi=4040)
    return make_case("restart_cuts", r, ell, M, "gen_cuts")


CASES = {}
for _ell in (2, 5):
    CASES["span%d_gen" % _ell] = (lambda ell=_ell: spans(ell, "gen"))
for _ell in (32, 33, 64, 65, 150, 256):
    for _form in ("ev", "gen"):
        CASES["span%d_%s" % (_ell, _form)] = (lambda ell=_ell, form=_form: spans(ell, form))
CASES.update({
    "M1_gen": lambda: spans(33, "gen", M=1),
    "M1_ev": lambda: spans(64, "ev", M=1),
    "span256_ev_M62": lambda: spans(256, "ev", M=62, seed=1),
    "span256_ev_M63_refused": lambda: spans(256, "ev", M=63, seed=1),
    "rounds_ev": lambda: many_rounds("ev", 32, 6, 2200, 3.0, 0.3, 3),
    "rounds_gen": lambda: many_rounds("gen", 65, 10, 1500, 2.5, 0.35, 4),
    "contigs_ev": lambda: contigs("ev"),
    "contigs_gen": lambda: contigs("gen"),
    "layout_over0": lambda: layout("over0"),
    "layout_over1": lambda: layout("over1"),
    "layout_over_many": lambda: layout("over_many"),
    "ties": ties,
    "prepick": prepick,
    "reach_far": lambda: reach("far"),
    "reach_cut": lambda: reach("cut"),
    "reach_none": lambda: reach("none"),
    "reach_none_later": lambda: reach("none_later"),
    "limit_others": limit_others,
    "limit_suspects": limit_suspects,
    "restart_ev": restart_ev,
    "restart_cuts": restart_cuts,
})
CASES = {key: (lambda key=key, build=build: dict(build(), name=key)) for key, build in CASES.items()}   # (named as pytest names them)
# the give-up cases, and the flag each ends on
GIVE_UP = {"span256_ev_M63_refused": "refused", "reach_none": 1, "reach_none_later": 1, "limit_others": 4, "limit_suspects": 2}
