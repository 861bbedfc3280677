"""The near-uniform route in the shape the DEVICE runs it (csrc/kernels/near_uniform.inc.hip): one function per stage of
tests/cpp/nu_stage_driver.hip, each leaving the expected content of every buffer that stage may write.  Plain numpy and
Python ints, any number of contigs on one global axis.  tests/near_uniform_model.py states the batched scheme itself
(solve_near_uniform_batched); this module states what the kernels make of it:

  0        the route's two looks at the spans (span_stats);
  setup    launch_nu_setup: the groups' scan, the dense order, ce (exclusive scan of the exceptions' coverage differences:
           exceptions covering p = ce[p + 1]), nadj, and the prepick (cov_all(start) <= M: selected on release);
  sweep    ALWAYS a whole sweep of every contig under the current nadj: need'(p) = min(cov_regular(p), M) + nadj[p],
           selend[p] = boff[p] + S(p).  The device's restarted chain (event-driven form, from a block that is a multiple of
           64) and its marked stretches (block-scan form under a cut-point table) must reproduce it: DESIGN.md 4.3 allows
           no stale position, so the model knows none.  The block-scan forms are the plain greedy (sweep_contig); the
           event-driven form is its kept-count recurrence (sweep_contig_events), which is the greedy as long as the
           greedy never holds a surplus and is not from a trial round's first surplus on: the rule, its three effects and
           where DESIGN.md states them are in that function's docstring, and sweep() logs every sweep against the greedy;
  round    launch_nu_round: k_nu_diff's dirty cells, the reset, what k_nu_verify lists and replays (swept_from, the dirty
           cells, the kept "no anchor" key), the cells' counts and starts, k_nu_replay with its two reaches (one span, then
           REACH), cut-point starts and the unresolved key, the key's bit layout, and k_nu_select_apply's nadj, pick,
           sweep_from, marks_next, dirty_next and state words;
  mark     launch_nu_mark_selected on a zeroed mask.

A Model holds the buffers under the driver's names; run(case) plays the driver's loop and returns the stages."""
import numpy as np

NOKEY = (1 << 64) - 1
UNPICKED = 0xFFFFFFFF
NONE32 = 0xFFFFFFFF
UNRESOLVED_LOW = 0x7FFFF
KEY_SHIFT = 19
OTHERS = 1024            # kNuOthers
REACH = 6                # kNuReach
GROUP = 128
CANARY32 = 0xA5A5A5A5
CANARY64 = 0xA5A5A5A5A5A5A5A5
MAX_WINDOWS_ONE_SPAN = 768   # sweep_plan.h: kSweepWindowsOneSpan
SEG_MAX_CANDIDATES = 4096    # sweep_plan.h: kSegMaxCandidates
MAX_SWEEP_WINDOWS = 3840     # sweep_plan.h: kMaxSweepWindows


def event_key(t, s, e, kind):
    """an open question's key: earlier time first, then the larger end, the larger start; kind 0 select, 1 unselect"""
    return (t << KEY_SHIFT) | ((511 - (e - t)) << 10) | ((t - s) << 1) | kind


def unresolved_key(s):
    return (s << KEY_SHIFT) | UNRESOLVED_LOW


def bin_shift(ltot):
    shift = 8
    while (ltot >> shift) + 1 > (1 << 17):
        shift += 1
    return shift


def segment_windows(ltot, ell, n_contigs):
    """sweep_plan.h: sweep_segment_windows"""
    if n_contigs >= 256 or ell == 0:
        return 0
    w = ltot // (64 * ell)
    cap = min(MAX_WINDOWS_ONE_SPAN, SEG_MAX_CANDIDATES - 256)
    return 0 if w < 2 else min(w, cap)


def sweep_supported(form, ell, M):
    """sweep_plan.h: the pipelined forms take spans up to 256; the event-driven form's packed field of 30 / E bits
    (E = ceil(ell / 64) words, the top bit a guard) must hold M + 1"""
    words = (ell + 63) // 64
    if ell < 1 or words > 4:
        return False
    return form != "ev" or M + 1 <= (1 << (30 // words - 1)) - 1


def segment_words(n_contigs, windows=MAX_SWEEP_WINDOWS):
    return windows + 3 * (1 + 5 * (n_contigs + windows))


def sweep_contig(c, need, ell, surplus=None):
    """the one-span greedy over counts (near_uniform_model.regular_sweep with a running window): S per bucket.
    surplus (a list, or None): receives every time at which the reads kept so far cover MORE than the need -- the need
    fell by more than the kept reads that expire; the greedy of a true need never holds one (what it has kept covers at
    most min(cov, M) of the next position), a trial round's need' may"""
    L = len(c)
    cur = [0] * L
    win = 0
    stack = []
    for t in range(L):
        if t - ell >= 0:
            win -= cur[t - ell]
        d = need[t] - win
        if d < 0 and surplus is not None:
            surplus.append(t)
        if c[t] > 0:
            stack.append(t)
        while d > 0 and stack:
            u = stack[-1]
            if u <= t - ell:       # (out of the window, and so is everything below it)
                del stack[:]
                break
            have = c[u] - cur[u]
            k = min(d, have)
            cur[u] += k
            win += k
            d -= k
            if k == have:
                stack.pop()
    return cur


def sweep_contig_events(c, need, ell, sat):
    """The event-driven form's recurrence (k_sweep_uniform_ev's general step), block by block on KEPT
    counts: the demand at p is need(p) - need(p - 1) + S(p - ell), served from bucket p and pushed back to p - 1, p - 2,
    ... (a suffix Lindley recursion over the block); what leaves the block's first position goes top-down through the
    free room of the block before, whose kept counts are this block's expiries -- repeated until nothing more is handed
    back.

    The recurrence is on DIFFERENCES of the need, so it is the greedy (sweep_contig) exactly as long as the kept reads
    cover the need and no more at every time -- true of any real need -- and it is NOT the greedy from the first time
    the greedy holds a SURPLUS (sweep_contig's `surplus`: need' fell by more than the kept reads that expire; only a
    trial round of the near-uniform route, whose need' carries a selection the sweep did not need, has one).  What the
    chain then does, all of it transcribed here because the device does it and the replay reads its result:
      1. the negative demand is clamped at zero and the surplus is forgotten (the kernel's comment at the clamp;
         DESIGN.md 7: "the event-driven chain clamps a negative demand at zero where a unit is applied before it is
         drawn on, and would have to carry that surplus forward"): from there on the chain asks for more than the greedy;
      2. the excess is served like any demand: from the window (more reads kept), or, where the window is used up,
         handed back through the WHOLE block before -- a read kept from a bucket that no longer covers the position
         ("unmet demand is handed back through the whole block before, beyond the positions that could
         have served it"); the cap of need' at cov_regular keeps a real need from ever doing that;
      3. what finds no room there either is dropped (`sum(room) < rem`: "cannot happen for a feasible demand; do not
         spin"), the block keeps the counts of the step before, and -- differences again -- the shortfall stays: the
         chain may then cover LESS than need' over hundreds of positions, until the coverage runs out.
    So after a surplus the chain may keep more reads or fewer than the greedy; before the first surplus, and in every
    round without one, it keeps exactly the greedy's.  The restart block and the checkpoints play no part: this is a
    whole sweep from block 0, and the device's restarted chain equals it word for word.
    Why the rounds still end on the greedy (an argument, not a proof; DESIGN.md 4.3 "Stage test" has it in full): the
    true greedy never holds a surplus, so the right selection is a fixed point the chain reproduces exactly; and a
    round's FIRST surplus, at time t, with everything before t certified, means that more is selected at t than the
    deficit there, so the selected exception of lowest priority at t fails "wanted at its time" and the round is not the
    last.  What the argument leaves open -- a hand-back after t that reaches a bucket the replay of an earlier question
    takes as final -- is held by assertion: tests/test_nu_stage_model_cpu.py pins that every sweep without a surplus
    equals sweep_contig, that every last round has none, which rounds of which cases differ and in which direction, and
    that every case ends on the oracle's selection."""
    L = len(c)
    S_all = [0] * L
    g = [0] * ell            # kept counts of the block before
    cprev = [0] * ell        # its counts, as the packed word holds them (saturated)
    for k in range((L + ell - 1) // ell):
        lo = k * ell
        n = min(ell, L - lo)
        cb = [c[lo + i] if i < n else 0 for i in range(ell)]
        dn = [(need[lo + i] - (need[lo + i - 1] if lo + i > 0 else 0)) if i < n else 0 for i in range(ell)]
        pushed = 0
        while True:
            d = [max(g[i] + dn[i], 0) if i < n else 0 for i in range(ell)]
            T, acc = [], 0
            for i in range(ell):
                acc += d[i] - cb[i]
                T.append(acc)
            suf = [0] * (ell + 1)          # suf[i] = max T[i..], none behind the last
            mx = None
            for i in range(ell - 1, -1, -1):
                mx = T[i] if mx is None else max(mx, T[i])
                suf[i] = mx
            ov = [max(0, suf[i] - (T[i - 1] if i > 0 else 0)) for i in range(ell)] + [0]
            S = [d[i] + ov[i + 1] - ov[i] for i in range(ell)]
            e = ov[0]
            if e == pushed:
                break
            rem = e - pushed
            pushed = e
            room = [max(cprev[i] - g[i], 0) for i in range(ell)]
            left = rem
            for i in range(ell - 1, -1, -1):
                take = min(room[i], left)
                g[i] += take
                left -= take
            if sum(room) < rem:
                break
        if k > 0:
            for i in range(ell):
                S_all[lo - ell + i] = g[i]
        for i in range(n):
            S_all[lo + i] = S[i]
        g = S[:]
        cprev = [min(v, sat) for v in cb]
    return S_all


class Model:
    def __init__(self, case):
        self.case = case
        self.ell, self.M = int(case["ell"]), int(case["M"])
        self.lengths = [int(v) for v in case["lengths"]]
        self.n_contigs = len(self.lengths)
        self.poff = [0]
        for v in self.lengths:
            self.poff.append(self.poff[-1] + v)
        self.ltot = self.poff[-1]
        self.form = case["form"]
        self.cap_sus = int(case["suspects_cap"])
        self.boff = [int(v) for v in case["boff"]]
        assert len(self.boff) == self.ltot + 1
        self.C = [self.boff[p + 1] - self.boff[p] for p in range(self.ltot)]
        # the list, in the dense order: the groups' filled slots, then the overflow region's
        self.cnt = [int(v) for v in case["cnt"]]
        self.n_groups = len(self.cnt)
        self.n_over = int(case["over"].shape[0])
        ent = [tuple(int(v) for v in row) for row in case["slots"]] + [tuple(int(v) for v in row) for row in case["over"]]
        self.gs = [t[0] for t in ent]
        self.ge = [t[1] for t in ent]
        self.idx = [t[2] for t in ent]
        self.n_exc = len(ent)
        self.place = []            # where each one's pick and key are dumped: ("g", slot) or ("o", k)
        for g, k in enumerate(self.cnt):
            self.place += [("g", g * GROUP + j) for j in range(k)]
        self.place += [("o", k) for k in range(self.n_over)]
        self.contig = [self.contig_of(s) for s in self.gs]
        self.shift = bin_shift(self.ltot)
        self.n_cells = (self.ltot >> self.shift) + 1
        self.windows = segment_windows(self.ltot, self.ell, self.n_contigs) if self.form == "gen_cuts" else 0
        self.n_cand = self.n_contigs + self.windows
        self.gen = self.form != "ev"
        # buffers
        self.pick = [CANARY32] * self.n_exc
        self.key = [CANARY64] * self.n_exc
        self.state = [0] * 16
        self.ce = [CANARY32] * (self.ltot + 3)
        self.nadj = [None] * (self.ltot + 1)
        self.selend = None
        self.prev = None
        self.viol_key = [CANARY64] * self.n_contigs
        self.viol_idx = [CANARY32] * self.n_contigs
        self.sweep_from = [[0] * self.n_contigs, [CANARY32] * self.n_contigs]    # physical buffers 0, 1
        self.marks = [[CANARY32] * self.n_cand, [CANARY32] * self.n_cand]
        fill = 0 if self.gen else CANARY32
        self.dirty = [[fill] * (self.n_cells + 1), [fill] * (self.n_cells + 1)]
        self.cur = 0               # which physical buffer is "this round's" (they change places after every round)
        self.seg = None            # the exact table's stretches [(start, end, contig end)]
        self.cuts = None
        # the lists: ids in the model's order, and how far any round has written
        self.listed, self.replayed, self.far, self.cells = [], [], [], {}
        self.high = {"suspects": 0, "sorted": 0, "replay": 0, "far": 0}
        self.bins_count = [CANARY32] * (self.n_cells + 1)
        self.bins_start = [CANARY32] * (self.n_cells + 2)
        self.mask = np.zeros((int(case["n"]) + 63) // 64, np.uint64)
        self.kept_total = 0
        self.questions = []        # per round: [(exception, kind)] applied
        self.sweeps = []           # per round: how the event-driven recurrence compares with the greedy (sweep())
        self.restarts = []         # per round: the block every contig's next sweep starts from
        self.seen = {}           # which of the replay's ways were taken, how often (for the cases' own checks)
        self.stopped_at_flag2 = False

    # ------------------------------------------------------------------------------------------------ small helpers
    def note(self, what):
        self.seen[what] = self.seen.get(what, 0) + 1

    def contig_of(self, pos):
        lo, hi = 0, self.n_contigs       # last c with poff[c] <= pos
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if self.poff[mid] <= pos:
                lo = mid
            else:
                hi = mid
        return lo

    def cell(self, pos):
        return min(pos >> self.shift, self.n_cells - 1)

    def cov_regular(self, p):
        return self.boff[p + 1] - self.boff[p + 1 - self.ell if p + 1 >= self.ell else 0]

    def S(self, u):
        return self.selend[u] - self.boff[u]

    def exhausted(self, u, c0):
        return u < c0 or self.S(u) == self.C[u]

    # ------------------------------------------------------------------------------------------------------ stage S
    def setup(self):
        ltot, ell, M = self.ltot, self.ell, self.M
        diff = [0] * (ltot + 3)
        for s, e in zip(self.gs, self.ge):
            diff[s] += 1
            diff[e + 1] -= 1
        acc = 0
        for q in range(ltot + 2):    # exclusive scan over ltot + 2 entries; the last word stays zero
            self.ce[q] = acc & 0xFFFFFFFF
            acc += diff[q]
        self.ce[ltot + 2] = 0
        for p in range(ltot):
            cr = self.cov_regular(p)
            self.nadj[p] = min(cr + self.ce[p + 1], M) - min(cr, M)
        self.nadj[ltot] = 0
        self.state = [0] * 16
        for x in range(self.n_exc):
            s, e = self.gs[x], self.ge[x]
            self.key[x] = NOKEY
            if self.cov_regular(s) + self.ce[s + 1] <= M:
                self.pick[x] = s
                self.state[3] += 1
            else:
                self.pick[x] = UNPICKED
        for x in range(self.n_exc):
            if self.pick[x] != UNPICKED:
                for p in range(self.gs[x], self.ge[x] + 1):
                    self.nadj[p] -= 1

    # ------------------------------------------------------------------------------------------------ stage "cuts"
    def find_cuts(self):
        """k_find_cuts and the exact table of k_build_segments: stretches start at non-empty contigs' first positions and
        at each window's first q with cov_all(q - 1) <= M that is no contig's first position"""
        ltot, nw = self.ltot, self.windows
        win = (ltot + nw - 1) // nw
        starts_of_contigs = set(self.poff[:self.n_contigs])
        self.cuts = []
        for w in range(nw):
            found = NONE32
            for q in range(max(w * win, 1), min((w + 1) * win, ltot)):
                cov = self.boff[q] - self.boff[q - self.ell if q >= self.ell else 0] + self.ce[q]
                if cov <= self.M and q not in starts_of_contigs:
                    found = q
                    break
            self.cuts.append(found)
        bounds = sorted([q for q in self.cuts if q != NONE32] +
                        [self.poff[c] for c in range(self.n_contigs) if self.lengths[c] > 0])
        self.seg = []
        for r, m in enumerate(bounds):
            cend = self.poff[self.contig_of(m) + 1]
            nxt = bounds[r + 1] if r + 1 < len(bounds) else ltot
            self.seg.append((m, min(nxt, cend), cend))

    def seg_words(self):
        out = np.full(segment_words(self.n_contigs), CANARY32, np.uint32)
        if self.seg is None:
            return out
        out[:self.windows] = self.cuts
        t = out[self.windows:]
        t[0] = len(self.seg)
        for r, (a, b, ce) in enumerate(self.seg):
            t[1 + 3 * r:4 + 3 * r] = (a, b, ce)
            t[1 + 3 * self.n_cand + r] = a
            t[1 + 4 * self.n_cand + r] = r
        return out

    # -------------------------------------------------------------------------------------------------- stage r.sweep
    def sweep(self):
        if self.selend is None:
            self.selend = [CANARY32] * self.ltot
        log = {"surplus": 0, "kept_more": 0, "equal": True}    # event-driven form: against the independent greedy
        self.sweeps.append(log)
        for c in range(self.n_contigs):
            a, b = self.poff[c], self.poff[c + 1]
            if self.gen:
                need = [min(self.cov_regular(p), self.M) + self.nadj[p] for p in range(a, b)]
                S = sweep_contig(self.C[a:b], need, self.ell)
            else:
                # capped at what the regular reads can give, as both kernels do (what cannot be met would be handed back
                # for good); the greedy above needs no cap -- it cannot keep more than there is, and drops the rest.
                # sat: the packed count field's maximum; no case has a bucket above it (63 at ell = 256), kept for the
                # transcription's sake
                need = [min(min(self.cov_regular(p), self.M) + self.nadj[p], self.cov_regular(p)) for p in range(a, b)]
                words = (self.ell + 63) // 64
                S = sweep_contig_events(self.C[a:b], need, self.ell, (1 << (30 // words - 1)) - 1)
                surplus = []
                G = sweep_contig(self.C[a:b], need, self.ell, surplus)
                log["surplus"] += len(surplus)
                log["kept_more"] += sum(S) - sum(G)
                log["equal"] = log["equal"] and S == G
            for p in range(a, b):
                self.selend[p] = self.boff[p] + S[p - a]

    # -------------------------------------------------------------------------------------------------- stage r.round
    def round(self, first):
        ell = self.ell
        cur, nxt = self.cur, 1 - self.cur
        dirty = None
        if self.gen:
            # k_nu_diff: cells whose kept counts differ from the round before, on top of what the last round's apply marked
            if not first:
                for p in range(self.ltot):
                    if self.selend[p] != self.prev[p]:
                        self.dirty[cur][self.cell(p)] = 1
            self.prev = list(self.selend)
            self.dirty[nxt] = [0] * (self.n_cells + 1)
            dirty = None if first else self.dirty[cur]
        dirty_next = self.dirty[nxt] if self.gen else None
        # k_nu_round_reset
        st = self.state
        st[7] = (1 if first else 0) | st[1]
        st[6] += 1 if st[1] != 0 else 0
        st[1] = st[4] = st[14] = st[15] = 0
        self.viol_key = [NOKEY] * self.n_contigs
        self.viol_idx = [NONE32] * self.n_contigs
        self.sweep_from[nxt] = [NONE32] * self.n_contigs
        if self.seg is not None:
            self.marks[nxt] = [0] * self.n_cand
        swept_from = self.sweep_from[cur]
        # k_nu_verify
        self.listed, self.replayed, self.far, self.cells = [], [], [], {}
        count = [0] * (self.n_cells + 1)
        if st[7] != 0:
            for x in range(self.n_exc):
                s, e = self.gs[x], self.ge[x]
                b = e - ell + 1
                c0 = self.poff[self.contig[x]]
                frm = swept_from[self.contig[x]]
                listed = not (frm == NONE32 or (e - c0) + ell < frm * ell)
                if listed and self.pick[x] == UNPICKED:
                    u = s
                    while u > b and listed:
                        listed = self.exhausted(u, c0)
                        u -= 1
                if not listed:
                    continue
                replay = (e - c0) >= frm * ell
                k0 = self.key[x]
                was_unresolved = dirty is not None and k0 != NOKEY and (k0 & UNRESOLVED_LOW) == UNRESOLVED_LOW
                if replay and dirty is not None and not was_unresolved:
                    c_lo = self.cell(max(s - (REACH + 1) * ell, 0))
                    c_hi = self.cell(e + 1)
                    replay = any(dirty[cc] != 0 for cc in range(c_lo, c_hi + 1))
                if was_unresolved and replay:
                    c_lo, c_hi = self.cell(max(s - (REACH + 1) * ell, 0)), self.cell(e + 1)
                    if not any(dirty[cc] != 0 for cc in range(c_lo, c_hi + 1)):
                        self.note("unresolved_again_no_dirty_cell")
                if not was_unresolved or replay:
                    self.key[x] = NOKEY
                else:
                    self.note("unresolved_key_kept")
                self.listed.append(x)
                if replay:
                    self.replayed.append(x)
            st[4] = len(self.listed)
            st[14] = len(self.replayed)
            if st[4] > self.cap_sus:
                # which ones the list holds is the order's: the flags, the count and the guards are all that is compared
                st[2] |= 2
                self.stopped_at_flag2 = True
                return
            for x in self.listed:
                cc = self.cell(self.gs[x])
                count[cc] += 1
                self.cells.setdefault(cc, []).append(x)
        self.bins_count = count
        acc = 0
        for cc in range(self.n_cells + 1):
            self.bins_start[cc] = acc
            acc += count[cc]
        self.high["suspects"] = max(self.high["suspects"], len(self.listed))
        self.high["sorted"] = max(self.high["sorted"], len(self.listed))
        self.high["replay"] = max(self.high["replay"], len(self.replayed))
        # k_nu_replay, one span of reach, then the far list with REACH
        by_contig = {}
        for x in self.listed:
            by_contig.setdefault(self.contig[x], []).append(x)
        for x in self.replayed:
            self.replay(x, False, by_contig[self.contig[x]])
        st[15] = len(self.far)
        self.high["far"] = max(self.high["far"], len(self.far))
        for x in self.far:
            self.replay(x, True, by_contig[self.contig[x]])
        # k_nu_select_apply
        applied = []
        pick_before = list(self.pick)
        for x in self.listed:
            k = self.key[x]
            c = self.contig[x]
            if k == NOKEY:
                continue
            if (k & UNRESOLVED_LOW) == UNRESOLVED_LOW:
                if k == self.viol_key[c]:
                    st[2] |= 1
                continue
            t, e = k >> KEY_SHIFT, self.ge[x]
            old = pick_before[x]
            if (k & 1) == 0:
                hi = old - 1 if old != UNPICKED else e
                for p in range(t, hi + 1):
                    self.nadj[p] -= 1
                self.pick[x] = t
                if old == UNPICKED:
                    st[3] += 1
                applied.append((x, "select" if old == UNPICKED else "earlier"))
            else:
                for p in range(old, e + 1):
                    self.nadj[p] += 1
                self.pick[x] = UNPICKED
                st[3] -= 1
                applied.append((x, "unselect"))
            c0 = self.poff[c]
            kt = (t - c0) // ell
            self.sweep_from[nxt][c] = min(self.sweep_from[nxt][c], (kt - 2 if kt >= 2 else 0) & ~63)
            if dirty_next is not None:
                for cc in range(self.cell(min(t, old)), self.cell(e) + 1):
                    dirty_next[cc] = 1
            if self.seg is not None:
                firstp = min(t, old)
                lo = firstp - ell + 1 if firstp - c0 >= ell else c0
                a = 0
                for r, sg in enumerate(self.seg):      # last stretch with start <= lo
                    if sg[0] <= lo:
                        a = r
                r = a
                while r < len(self.seg) and self.seg[r][0] <= e:
                    self.marks[nxt][r] = 1
                    r += 1
        st[1] = len(applied)
        st[3] &= 0xFFFFFFFF
        self.questions.append(applied)
        self.restarts.append(list(self.sweep_from[nxt]))
        self.cur = nxt    # the buffers change places

    def replay(self, x, far, neighbours):
        """k_nu_replay<far> for one listed exception: its key, the far list, flag 4, the contig's earliest key"""
        ell, M = self.ell, self.M
        s, e = self.gs[x], self.ge[x]
        b = e - ell + 1
        c = self.contig[x]
        c0 = self.poff[c]
        sel = -1 if self.pick[x] == UNPICKED else self.pick[x]
        my_idx = self.idx[x]
        others = []     # (start, end, selection time or -1, outranks this one)
        n_others = 0
        for z in neighbours:
            if z == x:
                continue
            zs, ze = self.gs[z], self.ge[z]
            if ze < s or zs > e:
                continue
            above = ze > e or (ze == e and (zs > s or (zs == s and self.idx[z] < my_idx)))
            zp = self.pick[z]
            if not above and zp == UNPICKED:
                continue
            n_others += 1
            others.append((zs, ze, -1 if zp == UNPICKED else zp, above))
        if n_others > OTHERS:
            self.state[2] |= 4
            self.note("too_many_others")
            return
        boff, nadj, C = self.boff, self.nadj, self.C

        def need(t):
            frm = max(t + 1 - ell, 0)
            return min(boff[t + 1] - boff[frm], M) + nadj[t]

        def sum_S(lo, hi):
            return sum(self.S(u) for u in range(lo, hi))

        reach = REACH if far else 1
        u1, cut = b + 1, -1
        while u1 - 1 >= c0 and self.exhausted(u1 - 1, c0) and s - (u1 - 1) < reach * ell:
            u1 -= 1
        no_anchor = u1 - 1 >= c0 and self.exhausted(u1 - 1, c0)
        if no_anchor:
            p = s - 1
            while p > s - reach * ell and p >= c0:
                if self.cov_regular(p) + self.ce[p + 1] <= M:
                    cut = p
                    break
                p -= 1
        if cut < 0 and no_anchor:
            if not far:
                self.far.append(x)
                self.note("far")
                return
            k = unresolved_key(s)
            self.note("unresolved")
            self.key[x] = k
            self.viol_key[c] = min(self.viol_key[c], k)
            return
        if cut >= 0:
            self.note("far_cut" if far else "cut")
        elif far:
            self.note("far_anchor" if u1 - 1 >= c0 else "far_contig_start")
        u1 = cut + 1 if cut >= 0 else max(u1, c0)
        anchor = u1 - 1
        has_anchor = cut < 0 and anchor >= c0
        base = max(cut - ell + 1, c0) if cut >= 0 else (anchor if has_anchor else c0)
        cur = [0] * (e - base + 18)
        stack_cap = (reach + 2) * ell + 16
        repl, stack = 0, []
        if has_anchor:
            d = need(anchor) - sum_S(max(anchor - ell + 1, 0), anchor)
            repl = min(max(d, 0), C[anchor])
            cur[0] = repl
            stack.append(anchor)
        fixed = 0 if cut >= 0 else sum_S(max(u1 - ell + 1, 0), base)
        if cut >= 0:
            repl = 0
            for u in range(base, cut + 1):
                cur[u - base] = C[u]
                if u > cut + 1 - ell:
                    repl += C[u]
        avail = 0
        key = NOKEY
        last = sel if sel >= 0 else e
        for t in range(u1, last + 1):
            raw = need(t) - fixed - repl
            d = max(raw, 0)
            ct = C[t]
            if t > b:
                avail += ct
            if t >= s:
                k = 1 if sel == t else 0
                r = 0
                for (zs, ze, zt, above) in others:
                    k += 1 if zt == t else 0
                    r += 1 if (above and zs <= t <= ze and (zt < 0 or zt >= t)) else 0
                wanted = raw + k > avail + r
                before = sel < 0 or t < sel
                if (wanted if before else not wanted):
                    key = event_key(t, s, e, 0 if before else 1)
                    break
            avail -= min(d, avail)
            if ct > 0 and len(stack) < stack_cap:
                stack.append(t)
            while d > 0 and stack:
                u = stack[-1]
                have = C[u] - cur[u - base]
                k = min(d, have)
                cur[u - base] += k
                repl += k
                d -= k
                if k == have:
                    stack.pop()
            if sel < 0 and t >= s and not self.exhausted(t, c0):
                break
            out = t - ell + 1
            if out >= base:
                repl -= cur[out - base]
            elif out >= 0 and cut < 0:
                fixed -= self.S(out)
        self.key[x] = key
        if key != NOKEY:
            self.viol_key[c] = min(self.viol_key[c], key)

    # ----------------------------------------------------------------------------------------------------- stage mark
    def mark(self):
        bits = np.zeros(self.mask.size * 64, bool)
        for x in range(self.n_exc):
            if self.pick[x] != UNPICKED:
                bits[self.idx[x]] = True
        self.kept_total = int(bits.sum())
        self.mask = np.packbits(bits.astype(np.uint8), bitorder="little").view("<u8").astype(np.uint64)

    # ------------------------------------------------------------------------------------- the buffers, as dumped
    def buffers(self):
        """every buffer of the dump, as a correct device would hand it back (lists: in the model's order; what the model
        does not specify -- spare words, stale list entries, debug words -- holds whatever: nu_stage_compare skips it)"""
        u32 = lambda v: np.array([w & 0xFFFFFFFF for w in v], np.uint32)  # noqa: E731
        u64 = lambda v: np.array(v, np.uint64)  # noqa: E731
        pick = np.full(self.n_groups * GROUP, CANARY32, np.uint32)
        key = np.full(self.n_groups * GROUP, CANARY64, np.uint64)
        pick_over = np.zeros(self.n_over, np.uint32)
        key_over = np.zeros(self.n_over, np.uint64)
        for x, (where, at) in enumerate(self.place):
            (pick if where == "g" else pick_over)[at] = self.pick[x]
            (key if where == "g" else key_over)[at] = self.key[x]
        goff = np.concatenate([[0], np.cumsum(self.cnt)]).astype(np.uint32)
        dense = np.array([(at if where == "g" else self.case["gcap"] + at) for where, at in self.place], np.uint32)
        cap = self.cap_sus
        lists = np.full(5 * cap, CANARY32, np.uint32)
        slot_of = {x: q for q, x in enumerate(self.listed)}
        n_sus = min(len(self.listed), cap)
        for q, x in enumerate(self.listed[:cap]):
            lists[2 * q], lists[2 * q + 1] = x_slot(self, x), self.contig[x]
        at = 0
        for cc in sorted(self.cells):
            assert at == self.bins_start[cc]
            for x in self.cells[cc]:
                lists[2 * cap + at] = slot_of[x]
                at += 1
        assert at == n_sus or self.stopped_at_flag2
        for q, x in enumerate(self.replayed[:cap]):
            lists[3 * cap + q] = slot_of[x]
        for q, x in enumerate(self.far[:cap]):
            lists[4 * cap + q] = slot_of[x]
        selend = np.full(self.ltot + 8, CANARY32, np.uint32)
        if self.selend is not None:
            selend[:self.ltot] = u32(self.selend)
        prev = np.full(self.ltot + 8, CANARY32, np.uint32)
        if self.prev is not None:
            prev[:self.ltot] = u32(self.prev)
        scalars = np.zeros(16, np.uint32)
        scalars[0], scalars[1] = self.kept_total & 0xFFFFFFFF, self.kept_total >> 32
        out = {"ce": u32(self.ce), "nadj": u32(self.nadj), "state": u32(self.state), "selend": selend, "lists": lists,
               "bins_count": u32(self.bins_count), "bins_start": u32(self.bins_start), "viol_key": u64(self.viol_key),
               "viol_idx": u32(self.viol_idx), "sweep_from0": u32(self.sweep_from[0]), "sweep_from1": u32(self.sweep_from[1]),
               "marks0": u32(self.marks[0]), "marks1": u32(self.marks[1]), "dirty0": u32(self.dirty[0]),
               "dirty1": u32(self.dirty[1]), "selend_prev": prev, "mask": self.mask.copy(), "scalars": scalars,
               "pick": pick, "pick_over": pick_over, "key": key, "key_over": key_over, "goff": goff,
               "goff_total": np.array([int(goff[-1])], np.uint32), "dense": dense}
        if self.form == "gen_cuts":
            out["segs"] = self.seg_words()
        return out

    def counts(self):
        """what nu_stage_compare needs beside the buffers: the lists' used lengths and how far any round has written"""
        cap = self.cap_sus
        return {"suspects": min(len(self.listed), cap), "replay": min(len(self.replayed), cap), "far": min(len(self.far), cap),
                "high": dict(self.high), "flag2": self.stopped_at_flag2}


def span_stats(case):
    """k_nu_count_span and k_nu_span_mode_share: reads of span ell; reads sampled (every one up to 64 Ki), reads in the
    fullest of 512 span bins (511: that or longer), the first such bin's span"""
    span = np.asarray(case["ends"], np.int64) - np.asarray(case["starts"], np.int64) + 1
    n = span.size
    stride = n // 65536 if n > 65536 else 1
    bins = np.bincount(np.minimum(span[::stride][:65536], 511), minlength=512)
    return np.array([int((span == int(case["ell"])).sum()), min((n + stride - 1) // stride, 65536), bins.max(), int(bins.argmax())], np.uint32)


def x_slot(m, x):
    where, at = m.place[x]
    return at if where == "g" else m.case["gcap"] + at


def run(case):
    """the driver's loop on the model -> {"stages": [(stage, buffers, counts)], "rounds", "flags", "settled", "model"}"""
    m = Model(case)
    stages = []

    def snap(stage):
        stages.append((stage, m.buffers(), m.counts()))

    stages.append(("0", {"span_stats": span_stats(case)}, None))
    m.setup()
    snap("S")
    if m.form == "gen_cuts":
        if m.windows == 0:
            return {"stages": stages, "refused": True, "rounds": 0, "flags": 0, "settled": False, "model": m}
        m.find_cuts()
        snap("cuts")
    refuses = not sweep_supported(m.form, m.ell, m.M)
    rounds, settled = 0, False
    while rounds < int(case["rounds_max"]) and not settled:
        rounds += 1
        if refuses:
            return {"stages": stages, "refused": True, "rounds": rounds, "flags": 0, "settled": False, "model": m}
        m.sweep()
        snap("%d.sweep" % rounds)
        m.round(rounds == 1)
        snap("%d.round" % rounds)
        if m.state[2] != 0:
            break
        settled = m.state[1] == 0
    if settled:
        m.mark()
        snap("mark")
    return {"stages": stages, "refused": False, "rounds": rounds, "flags": m.state[2], "settled": settled, "model": m}
