"""Tables at the edges of the multi-GPU exchange step (sgtd_amd/csrc/exchange_kernels.hip.h) and restatements of its
rules.  Plain helper module of tests/test_exchange_edges.py (CPU: merge_ref is dist.merge_candidates on every case, every
mutant below changes the expected result on the cases named for it, every case's precondition holds) and
tests/test_gpu_exchange_edges.py (GPU: every entry point equals the restatements on them, word for word).  numpy only: no
device, no project code.

merge_ref is the reference's loop (STDesc.cpp:423-433) written literally: a vote count per frame id, candidate_num rounds
of "the strictly largest count, the first such frame in ascending frame order, stop below min_votes, clear the winner".
A case is a list of tables: cases()[name] = [dict(frames [W, Q, cn], votes [W, Q, cn], cn, flag_table, nq_word, cn_word,
pre, note)], where pre(table) -> bool is the precondition the table relies on (what makes it the edge it is named for) and
flag_table / nq_word / cn_word are packed()'s arguments.  Item i = table * cn + slot of a query sits in lane i % 64 and
register i // 64 of the merge kernel's wave; the kernel holds 1, 4, 8 or 16 registers per lane (PER) by n_tables * cn.

The per_* tables: a table group of ONE rank holds n_keys = cn keys, so "more than cn keys qualify" cannot hold for (1, 64);
there all 64 qualify and all 64 win.

The mutants (MUTANT_CASES names the cases that show each):
  tie_high        ties go to the highest frame id
  min_votes_4/_6  a frame needs 4 / 6 votes
  stop_early      the rounds stop after cn - 1
  first_64        only the first 64 items (register 0) are seen
  lane_gives_up   once a lane's best key is taken the lane's other keys are lost
  no_frame_check  a slot with frame -1 and votes counts
  src_merged_pos  src names the position in the merged list instead of the slot in the owner's table
  keep_table0     keep is taken from table 0, whatever my_table is
  flags_table0    only table 0's flag words are read
  flags_nq_only   of a table's shape words only nq is compared
None of the listed mutants had to be dropped."""
import functools

import numpy as np

M31 = 2 ** 31 - 1
FLAG_WORDS = 4
MINUS_ONE = np.array([-1.0]).view(np.uint64)[0]
SPECIAL_ITEMS = (0, 15, 16, 31, 32, 47, 48, 63, 64)
PER_SHAPES = {"per_64": ((1, 64), (64, 1)), "per_65": ((5, 13), (65, 1)), "per_256": ((4, 64),), "per_257": ((257, 1),),
              "per_512": ((8, 64),), "per_513": ((27, 19), (513, 1)), "per_1024": ((16, 64), (1024, 1))}
QUERY_COUNTS = (0, 1, 3, 4, 5, 257)
MERGE_MUTANTS = ("tie_high", "min_votes_4", "min_votes_6", "stop_early", "first_64", "lane_gives_up", "no_frame_check",
                 "src_merged_pos", "keep_table0")
FLAG_MUTANTS = ("flags_table0", "flags_nq_only")
MUTANT_CASES = {
    "tie_high": ("ties", "extremes"), "min_votes_4": ("threshold", "full_and_empty"), "min_votes_6": ("threshold", "query_counts"),
    "stop_early": tuple(PER_SHAPES) + ("full_and_empty", "keep_bits"),
    "first_64": ("per_65", "per_256", "per_257", "per_512", "per_513", "per_1024", "same_lane", "keep_bits"),
    "lane_gives_up": ("same_lane", "per_256", "per_512"), "no_frame_check": ("threshold",),
    "src_merged_pos": ("ties", "keep_bits", "per_256", "per_512", "same_lane"), "keep_table0": ("keep_bits", "ties", "full_and_empty"),
    "flags_table0": ("flags",), "flags_nq_only": ("flags",),
}
MUTANTS = tuple(MUTANT_CASES)
OUT_KEYS = ("frame", "votes", "n_cand", "src", "keep", "flags")


def per_of(n_keys):
    """key registers per lane the host picks for n_keys = n_tables * cn (None: refused)"""
    return 1 if n_keys <= 64 else 4 if n_keys <= 256 else 8 if n_keys <= 512 else 16 if n_keys <= 1024 else None


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


# ---- the restatements ----
def _merge_query(fr, vo, cn, min_votes, mutant):
    """one query, fr / vo [W, cn] -> [(frame, votes, item of the slot that held it)] in the order they are picked"""
    n_tables = fr.shape[0]
    count, holder = {}, {}
    for i in range(n_tables * cn):
        if mutant == "first_64" and i >= 64:
            break
        f, v = int(fr[i // cn, i % cn]), int(vo[i // cn, i % cn])
        if (f >= 0 or mutant == "no_frame_check") and v > 0:
            assert count.get(f, v) == v, "one frame with two vote counts"
            if f not in count:
                count[f], holder[f] = v, i
    order = sorted(count)
    need = {"min_votes_4": 4, "min_votes_6": 6}.get(mutant, min_votes)
    out = []
    for _ in range(cn - 1 if mutant == "stop_early" else cn):
        max_vote, best = 1, None
        for f in order:
            if count[f] > max_vote or (mutant == "tie_high" and count[f] == max_vote and best is not None):
                max_vote, best = count[f], f
        if best is None or max_vote < need:
            break
        count[best] = 0
        out.append((best, max_vote, holder[best]))
        if mutant == "lane_gives_up":
            for f in order:
                if holder[f] % 64 == holder[best] % 64:
                    count[f] = 0
    return out


def merge_with(frames, votes, cn, my_table, min_votes=5, mutant=None):
    """merge_ref with the part named by `mutant` replaced (None: the rule)"""
    assert mutant is None or mutant in MERGE_MUTANTS, mutant
    frames, votes = np.asarray(frames, np.int32), np.asarray(votes, np.int32)
    n_tables, nq, c = frames.shape
    assert c == cn and votes.shape == frames.shape
    out_f = np.full((nq, cn), -1, np.int32)
    out_v = np.zeros((nq, cn), np.int32)
    out_n = np.zeros(nq, np.int32)
    src = np.full((nq, cn), -1, np.int32)
    keep = np.zeros(nq, np.uint64)
    mine = 0 if mutant == "keep_table0" else my_table
    for q in range(nq):
        picked = _merge_query(frames[:, q], votes[:, q], cn, min_votes, mutant)
        out_n[q] = len(picked)
        word = 0
        for k, (f, v, item) in enumerate(picked):
            t, s = item // cn, item % cn
            out_f[q, k], out_v[q, k] = f, v
            src[q, k] = (t << 8) | (k if mutant == "src_merged_pos" else s)
            if t == mine:
                word |= 1 << s
        keep[q] = word
    return out_f, out_v, out_n, src, keep


def merge_ref(frames, votes, cn, my_table, min_votes=5):
    """frames, votes [W, Q, cn] -> frame [Q, cn], votes [Q, cn], n_cand [Q], src [Q, cn] (table << 8 | slot of the slot
    that held the winner), keep u64 [Q] (bit slot for the winners of my_table); unused rows are -1 / 0 / -1"""
    return merge_with(frames, votes, cn, my_table, min_votes)


def packed(frames, votes, flag_table=None, nq=None, cn=None, serial=7, stride_pad=0):
    """the int32 array an all-gather of the tables delivers: per table frames | votes | [overflow, nq, cn, serial]
    (| stride_pad ints of -9: the library's call takes tables back to back, stride_pad = 0).  flag_table: the table(s)
    whose overflow word is set; nq / cn: the shape words, for all tables (an int) or for single ones ({table: value})"""
    frames, votes = np.asarray(frames, np.int32), np.asarray(votes, np.int32)
    n_tables, q, c = frames.shape
    flagged = () if flag_table is None else (flag_table,) if np.isscalar(flag_table) else tuple(flag_table)

    def word(given, t, default):
        if given is None:
            return default
        return given.get(t, default) if isinstance(given, dict) else given

    rows = []
    for t in range(n_tables):
        rows += [frames[t].reshape(-1), votes[t].reshape(-1),
                 np.array([1 if t in flagged else 0, word(nq, t, q), word(cn, t, c), serial], np.int32), np.full(stride_pad, -9, np.int32)]
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)


def unpacked(arr, n_tables, nq, cn, stride_pad=0):
    """packed()'s inverse -> frames, votes [W, Q, cn], flag words [W, 4]"""
    a = np.asarray(arr, np.int32).reshape(n_tables, 2 * nq * cn + FLAG_WORDS + stride_pad)
    return (a[:, :nq * cn].reshape(n_tables, nq, cn).copy(), a[:, nq * cn:2 * nq * cn].reshape(n_tables, nq, cn).copy(),
            a[:, 2 * nq * cn:2 * nq * cn + FLAG_WORDS].copy())


def flags_with(arr, n_tables, nq, cn, stride_pad=0, mutant=None):
    """flags[0] of a merge over the packed tables: bit 0 some table's overflow word is set, bit 1 some table's shape words
    are not (nq, cn)"""
    assert mutant is None or mutant in FLAG_MUTANTS, mutant
    words = unpacked(arr, n_tables, nq, cn, stride_pad)[2]
    bad = 0
    for t in range(1 if mutant == "flags_table0" else n_tables):
        if words[t, 0] != 0:
            bad |= 1
        if words[t, 1] != nq or (mutant != "flags_nq_only" and words[t, 2] != cn):
            bad |= 2
    return bad


def flags_ref(arr, n_tables, nq, cn, stride_pad=0):
    return flags_with(arr, n_tables, nq, cn, stride_pad)


def gather_ref(gathered, src, nq, cn):
    """gathered [W, Q*cn*13] uint64 bit patterns (per table score [Q*cn] | pose [Q*cn*12]), src [Q, cn] -> score [Q, cn],
    pose [Q, cn, 12] as bit patterns; src < 0: the bits of -1.0 and +0.0"""
    g = np.asarray(gathered, np.uint64)
    g = g.reshape(-1, nq * cn * 13) if nq * cn else np.zeros((0, 0), np.uint64)
    src = np.asarray(src, np.int32).reshape(nq, cn)
    score = np.full((nq, cn), MINUS_ONE, np.uint64)
    pose = np.zeros((nq, cn, 12), np.uint64)
    for q in range(nq):
        for k in range(cn):
            s = int(src[q, k])
            if s < 0:
                continue
            t, j = s >> 8, q * cn + (s & 255)
            score[q, k] = g[t, j]
            pose[q, k] = g[t, nq * cn + j * 12:nq * cn + j * 12 + 12]
    return score, pose


def search_loop_ref(frames, n_cand, scores, icp_threshold):
    """the loop of STDesc.cpp:105-146 per query -> (best_cand, best_frame, best_score): -1 / -1 / 0 for "no loop" """
    out = []
    for q in range(len(n_cand)):
        best_score, best_frame, trigger = 0.0, -1, -1
        for i in range(int(n_cand[q])):
            if scores[q][i] > best_score:
                best_score, best_frame, trigger = float(scores[q][i]), int(frames[q][i]), i
        out.append((trigger, best_frame, best_score) if best_score > icp_threshold else (-1, -1, 0.0))
    return out


# ---- results of a case ----
def my_tables(n_tables):
    return sorted({0, n_tables - 1, -1})


def packed_of(t):
    return packed(t["frames"], t["votes"], t["flag_table"], t["nq_word"], t["cn_word"])


_expected = {}


def expected(t, my_table, mutant=None):
    """every output of a merge over the table -> dict of OUT_KEYS (computed once and left unchanged)"""
    key = (id(t), my_table, mutant)
    if key not in _expected:
        n_tables, nq, cn = t["frames"].shape
        m = merge_with(t["frames"], t["votes"], cn, my_table, mutant=mutant if mutant in MERGE_MUTANTS else None)
        f = flags_with(packed_of(t), n_tables, nq, cn, mutant=mutant if mutant in FLAG_MUTANTS else None)
        _expected[key] = dict(zip(OUT_KEYS, m + (f,)))
    return _expected[key]


def differs(t, mutant):
    """the outputs (over my_table 0, last, -1) that the mutant changes on the table"""
    out = []
    for my in my_tables(t["frames"].shape[0]):
        a, b = expected(t, my), expected(t, my, mutant)
        out += [(my, k) for k in OUT_KEYS if not np.array_equal(a[k], b[k])]
    return out


def items_of(t, q, my_table=-1):
    """items (table * cn + slot) of query q's winners, in the order they are picked"""
    e = expected(t, my_table)
    cn = t["cn"]
    return [int(s >> 8) * cn + int(s & 255) for s in e["src"][q, :e["n_cand"][q]]]


def qualifiers(t, q, min_votes=5):
    return int(((t["frames"][:, q] >= 0) & (t["votes"][:, q] >= min_votes)).sum())


# ---- builders ----
def _empty(n_tables, nq, cn):
    return np.full((n_tables, nq, cn), -1, np.int32), np.zeros((n_tables, nq, cn), np.int32)


def _put(fr, vo, q, item, frame, votes):
    cn = fr.shape[2]
    fr[item // cn, q, item % cn], vo[item // cn, q, item % cn] = frame, votes


def _table(fr, vo, pre, note="", flag_table=None, nq_word=None, cn_word=None, **extra):
    return dict(frames=fr, votes=vo, cn=fr.shape[2], flag_table=flag_table, nq_word=nq_word, cn_word=cn_word, pre=pre, note=note, **extra)


def _background(fr, vo, q, rng, spread):
    """every slot of query q a qualifying key: distinct frames in an order unrelated to the items, votes 5 .. 4 + spread"""
    n_tables, _, cn = fr.shape
    perm = rng.permutation(n_tables * cn)
    for i in range(n_tables * cn):
        _put(fr, vo, q, i, 3 * int(perm[i]) + 1, 5 + int(perm[i]) % spread)


def specials_of(n_keys):
    s = [i for i in SPECIAL_ITEMS if i < n_keys]
    return s + [n_keys - 1] if n_keys - 1 not in s else s


def _per(n_tables, cn):
    """query k: the strongest key at the k-th special item, the other specials behind it in rotated order, everything else
    weaker and qualifying; the last query: the specials tied, so the frame ids order them"""
    n = n_tables * cn
    sp = specials_of(n)
    fr, vo = _empty(n_tables, len(sp) + 1, cn)
    rng = np.random.default_rng(1000 * n + cn)
    for q in range(len(sp) + 1):
        _background(fr, vo, q, rng, 4)
        for r, i in enumerate(sp[q:] + sp[:q]):
            vo[i // cn, q, i % cn] = 1000 - r if q < len(sp) else 500

    def pre(t):
        for q in range(len(sp) + 1):
            if qualifiers(t, q) != n or not (n > cn or n_tables == 1):
                return False
            won = items_of(t, q)
            head = min(cn, len(sp))
            if q < len(sp) and won[:head] != (sp[q:] + sp[:q])[:head]:
                return False
            if q == len(sp):
                by_frame = sorted(sp, key=lambda i: int(t["frames"][i // cn, q, i % cn]))
                if won[:head] != by_frame[:head] or by_frame == sorted(sp):
                    return False
        return per_of(n) == {64: 1, 65: 4, 256: 4, 257: 8, 512: 8, 513: 16, 1024: 16}[n]

    return _table(fr, vo, pre, "%d x %d" % (n_tables, cn))


SAME_LANES = (0, 37, 63)


def _same_lane(n_tables, cn):
    """per query the 2, 3 and PER strongest keys in ONE lane (items l + 64 j), their votes rising or falling with the
    register; for lane 0 in the first registers, for the other lanes in the last ones"""
    n = n_tables * cn
    per = per_of(n)
    assert n == 64 * per and cn == 64
    runs = [(r, desc, lane) for r in (2, 3, per) for desc in (False, True) for lane in SAME_LANES]
    fr, vo = _empty(n_tables, len(runs), cn)
    rng = np.random.default_rng(77 + per)
    want = []
    for q, (r, desc, lane) in enumerate(runs):
        _background(fr, vo, q, rng, 3)
        regs = list(range(r)) if lane == 0 else list(range(per - r, per))
        items = [lane + 64 * j for j in regs]
        for k, i in enumerate(items):
            vo[i // cn, q, i % cn] = 100 + (r - k if desc else k)
        want.append(items if desc else items[::-1])

    def pre(t):
        return all(items_of(t, q)[:len(w)] == w and len({i % 64 for i in w}) == 1 and t["votes"][:, q].max() >= 100 and
                   int((t["votes"][:, q] >= 100).sum()) == len(w) for q, w in enumerate(want))

    return _table(fr, vo, pre, "PER %d" % per)


TIED = ((0, 0, 50), (0, 1, 10), (0, 2, 70), (1, 0, 40), (1, 1, 80), (1, 2, 20), (2, 0, 30), (2, 1, 60))     # (table, slot, frame)


def _ties():
    cn = 5
    fr, vo = _empty(3, 4, cn)
    _background(fr, vo, 0, np.random.default_rng(5), 1)              # every key at 5 votes
    for q in (1, 2):
        for t, s, f in TIED:                                         # cn + 3 frames with 9 votes over three tables
            fr[t, q, s], vo[t, q, s] = f, 9
    fr[2, 2, 4], vo[2, 2, 4] = 99, 12                                # two stronger: the cut at cn falls further into the tie
    fr[0, 2, 4], vo[0, 2, 4] = 98, 11
    for (t, s), (f, v) in {(0, 0): (5, 8), (0, 1): (3, 8), (1, 0): (4, 8), (1, 3): (1, 6), (2, 2): (2, 6)}.items():
        fr[t, 3, s], vo[t, 3, s] = f, v

    def pre(t):
        e = expected(t, -1)
        low = sorted(f for _, _, f in TIED)
        all5 = sorted(t["frames"][:, 0].reshape(-1).tolist())
        return (len(TIED) == cn + 3 and e["frame"][0].tolist() == all5[:cn] and e["frame"][1].tolist() == low[:cn]
                and {int(s) >> 8 for s in e["src"][1]} == {0, 1, 2} and e["frame"][2].tolist() == [99, 98] + low[:cn - 2]
                and e["frame"][3].tolist() == [3, 4, 5, 1, 2] and e["votes"][3].tolist() == [8, 8, 8, 6, 6])

    return _table(fr, vo, pre)


THRESHOLD_N = [0, 1, 2, 4, 0, 2, 1, 0]


def _threshold():
    cn = 4
    fr, vo = _empty(2, 8, cn)
    rows = {0: [(0, 10, 4), (3, 11, 4), (5, 12, 4)],                       # 4 alone
            1: [(6, 20, 5)],                                               # 5 alone
            2: [(1, 30, 6), (4, 31, 6)],                                   # 6 alone
            3: [(0, 40, 4), (1, 41, 5), (2, 42, 6), (4, 43, 4), (5, 44, 6), (7, 45, 5)],
            4: [(0, 50, 4), (1, 51, 3), (4, 52, 2), (6, 53, 1)],           # the best is exactly 4
            5: [(2, 60, 5), (5, 61, 5)],                                   # the only keys are at exactly 5
            6: [(0, 70, 0), (1, -1, 9), (5, 71, 6)],                       # a frame without votes, votes without a frame
            7: [(3, -1, 9), (4, 72, 0)]}
    for q, keys in rows.items():
        for item, f, v in keys:
            _put(fr, vo, q, item, f, v)

    def pre(t):
        e = expected(t, -1)
        return (e["n_cand"].tolist() == THRESHOLD_N and e["frame"][3].tolist() == [42, 44, 41, 45] and e["frame"][6].tolist() == [71, -1, -1, -1]
                and int(t["votes"][:, 4].max()) == 4 and bool(((t["frames"] == -1) & (t["votes"] == 9)).any())
                and bool(((t["frames"] >= 0) & (t["votes"] == 0)).any()))

    return _table(fr, vo, pre)


def _extremes():
    cn = 3
    fr, vo = _empty(2, 3, cn)
    for q, keys in {0: [(0, M31, 7), (5, 0, 7)], 1: [(1, M31, M31), (3, 0, 5), (4, 5, M31)], 2: [(2, 0, M31), (5, M31, 5)]}.items():
        for item, f, v in keys:
            _put(fr, vo, q, item, f, v)

    def pre(t):
        e = expected(t, -1)
        return (e["frame"].tolist() == [[0, M31, -1], [5, M31, 0], [0, M31, -1]]
                and e["votes"].tolist() == [[7, 7, 0], [M31, M31, 5], [M31, 5, 0]])

    return _table(fr, vo, pre)


def _full_and_empty(hole):
    """three tables of which table `hole` is all -1 / 0: no key at all, exactly cn qualifiers, cn - 1, twice cn"""
    cn = 4
    fr, vo = _empty(3, 4, cn)
    live = [t for t in range(3) if t != hole]
    keys = {1: [(9, 7), (8, 5), (7, 9), (6, 6), (5, 4), (4, 3)], 2: [(9, 5), (8, 8), (7, 5), (6, 4), (5, 4)],
            3: [(90 - k, 5 + k % 3) for k in range(8)]}
    for q, ks in keys.items():
        for k, (f, v) in enumerate(ks):
            fr[live[k % 2], q, k // 2], vo[live[k % 2], q, k // 2] = f, v

    def pre(t):
        e = expected(t, -1)
        return ([qualifiers(t, q) for q in range(4)] == [0, cn, cn - 1, 2 * cn] and e["n_cand"].tolist() == [0, cn, cn - 1, cn]
                and bool((t["frames"][hole] == -1).all()) and bool((t["votes"][hole] == 0).all()) and bool((t["frames"][:, 0] == -1).all()))

    return _table(fr, vo, pre, "empty table %d" % hole)


def _keep_bits():
    cn = 64
    fr, vo = _empty(3, 4, cn)
    rng = np.random.default_rng(64)
    for q in range(4):
        _background(fr, vo, q, rng, 3)
    vo[0, 0, 63], vo[2, 0, 63], vo[1, 0, 63] = 90, 80, 70                  # slot 63 of every table wins
    vo[0, 1] += 20                                                         # all of table 0 wins
    vo[2, 2] += 20                                                         # all of the last table wins
    vo[:, 3] = 5 + rng.integers(0, 26, (3, cn))

    def pre(t):
        first, last, none = expected(t, 0), expected(t, 2), expected(t, -1)
        top = np.uint64(1 << 63)
        full = np.uint64(2 ** 64 - 1)
        return (bool(first["keep"][0] & top) and bool(last["keep"][0] & top) and first["src"][0, :3].tolist() == [63, 2 << 8 | 63, 1 << 8 | 63]
                and first["keep"][1] == full and last["keep"][1] == 0 and last["keep"][2] == full and first["keep"][2] == 0
                and 0 < bin(int(first["keep"][3])).count("1") < 64 and not none["keep"].any() and bool((first["n_cand"] == 64).all()))

    return _table(fr, vo, pre)


def _query_counts(nq):
    """rows of five kinds by q % 5, the frame ids carry q: a row read at another query's offset shows"""
    cn = 3
    fr, vo = _empty(2, nq, cn)
    kinds = {0: [(0, 9), (1, 8), (2, 7), (3, 9), (4, 8), (5, 7)], 1: [], 2: [(5, 6)], 3: [(1, 5), (3, 11)], 4: [(0, 5), (2, 5), (3, 5), (4, 5)]}
    for q in range(nq):
        for item, v in kinds[q % 5]:
            _put(fr, vo, q, item, 100 * q + 50 - item, v)

    def pre(t):
        e = expected(t, -1)
        return t["frames"].shape == (2, nq, cn) and e["n_cand"].tolist() == [(3, 0, 1, 2, 3)[q % 5] for q in range(nq)] and e["flags"] == 0

    return _table(fr, vo, pre, "nq %d" % nq)


def _flags():
    fr, vo = _empty(3, 2, 2)
    for q in range(2):
        for item, (f, v) in enumerate([(7, 6), (3, 9), (8, 5), (1, 9), (5, 7), (2, 4)]):
            _put(fr, vo, q, item, f + 10 * q, v)
    out = []
    for want, kw in ((1, dict(flag_table=0)), (1, dict(flag_table=1)), (1, dict(flag_table=2)), (2, dict(nq_word={1: 3})),
                     (2, dict(cn_word={2: 3})), (3, dict(flag_table=1, cn_word={2: 1})), (3, dict(flag_table=(0, 1, 2), nq_word={2: 0})), (0, {})):
        out.append(_table(fr, vo, (lambda t, want=want: expected(t, -1)["flags"] == want and expected(t, -1)["n_cand"].tolist() == [2, 2]),
                          "flags %d %s" % (want, sorted(kw)), **kw))
    return out


def _equal_keys():
    """(frame 500, 20 votes) in both tables.  Query 0: table 0 holds it in lane 30, table 1 in lane 10 (item 74); query 1:
    table 0 in lane 3, table 1 in lane 50.  Stronger and weaker keys around it"""
    cn = 40
    fr, vo = _empty(2, 2, cn)
    where = {0: (30, 40 + 34), 1: (3, 40 + 10)}
    for q, pair in where.items():
        for i in pair:
            _put(fr, vo, q, i, 500, 20)
        for k, i in enumerate((0, 39, 41, 79, 20, 60)):
            _put(fr, vo, q, i, 100 + k, 25 - 2 * k)                        # 25, 23, 21 above the pair, 19, 17, 15 below

    def pre(t):
        ok = where[0][0] % 64 > where[0][1] % 64 and where[1][0] % 64 < where[1][1] % 64
        for q, pair in where.items():
            held = [(int(t["frames"][i // cn, q, i % cn]), int(t["votes"][i // cn, q, i % cn])) for i in pair]
            ok = ok and held == [(500, 20)] * 2 and pair[0] // cn == 0 and pair[1] // cn == 1
        return ok and expected(t, -1)["frame"][:, :7].tolist() == [[100, 101, 102, 500, 103, 104, 105]] * 2

    return _table(fr, vo, pre, holders=where)


@functools.lru_cache(None)
def cases():
    """name -> list of tables"""
    out = {name: [_per(w, cn) for w, cn in shapes] for name, shapes in PER_SHAPES.items()}
    out["same_lane"] = [_same_lane(4, 64), _same_lane(16, 64)]
    out["ties"] = [_ties()]
    out["threshold"] = [_threshold()]
    out["extremes"] = [_extremes()]
    out["full_and_empty"] = [_full_and_empty(hole) for hole in (0, 1, 2)]
    out["keep_bits"] = [_keep_bits()]
    out["query_counts"] = [_query_counts(nq) for nq in QUERY_COUNTS]
    out["flags"] = _flags()
    out["equal_keys"] = [_equal_keys()]
    return out


def candidate_nums():
    return sorted({t["cn"] for ts in cases().values() for t in ts})


# ---- sgtd_gather_verified_dev ----
DOUBLES = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF80000DEADBEEF, 0xFFF4000000C0FFEE, 0x7FF0000000000001,
                    0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000, 0xBFF0000000000000, 0], np.uint64)
# -0.0, +inf, -inf, NaNs with payloads (quiet, negative quiet, signalling), the smallest and the largest denormals, +-1.0, +0.0


@functools.lru_cache(None)
def gather_cases():
    """name -> dict(n_tables, nq, cn, gathered [W, Q*cn*13] uint64, src [Q, cn]): every third word one of DOUBLES in
    rotation, the others random bit patterns"""
    out = {}

    def add(name, n_tables, nq, cn, src):
        rng = np.random.default_rng(len(out) + 1)
        n = n_tables * nq * cn * 13
        g = rng.integers(0, 2 ** 64, n, dtype=np.uint64, endpoint=False)
        g[::3] = DOUBLES[(np.arange(len(g[::3])) * 5) % DOUBLES.size]
        out[name] = dict(n_tables=n_tables, nq=nq, cn=cn, gathered=g.reshape(n_tables, nq * cn * 13), src=np.asarray(src, np.int32).reshape(nq, cn))

    def mixed(n_tables, nq, cn, seed):
        rng = np.random.default_rng(seed)
        src = (rng.integers(0, n_tables, (nq, cn)) << 8) | rng.integers(0, cn, (nq, cn))
        src[rng.random((nq, cn)) < 0.2] = -1
        if nq:
            src[-1, -1] = (n_tables - 1) << 8 | (cn - 1)
            src[0, 0] = 0
        return src

    add("all_unused", 3, 6, 5, np.full((6, 5), -1))
    add("last_slot", 3, 6, 5, np.full((6, 5), 2 << 8 | 4))
    add("last_slot_cn64", 2, 3, 64, np.full((3, 64), 1 << 8 | 63))
    add("table_1023", 1024, 3, 1, [[1023 << 8], [512 << 8], [255 << 8]])
    add("n255", 3, 51, 5, mixed(3, 51, 5, 255))
    add("n256", 3, 64, 4, mixed(3, 64, 4, 256))
    add("n257", 3, 257, 1, mixed(3, 257, 1, 257))
    add("one_table", 1, 2, 4, mixed(1, 2, 4, 9))
    add("nq0", 2, 0, 4, np.zeros((0, 4)))
    return out
