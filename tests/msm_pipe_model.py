"""Plain-Python models of the stages of the large MSM (bls12_381_amd/csrc/msm.hip.h, driven by api_msm.hip msm_device): the signed
c-bit recoding, the bucket multiset per (window, bucket), the sort's key split, the work-item partition and the level sums of the
window reduction.  Big integers and lists only, nothing from the library: tests/test_simt_msm_front.py compares the emulated kernels
with them, tests/test_msm_pipeline_gpu.py builds its scalars with them.  Test infrastructure only: the product never imports this file.
"""

# limits restated from the product (a test pins each of them against the header it comes from)
SORT_TILE = 4096                 # msm.hip.h BLS_SORT_TILE
SORT_MAX_COUNTERS = 8192         # msm.hip.h
ITEM_CAP_MAX = 4096              # limits.h
ITEM_BLOCK_BUCKETS = 2048        # msm.hip.h: 256 * ITEM_PER_THREAD
HEAVY_SMALL = 16                 # msm.hip.h
HEAVY_BIG_BLOCKS = 512           # msm.hip.h
WINDOW_RANGE = (4, 16)           # api_ctx.hip blsgpu_set_msm_window
TABLE_WINDOW_RANGE = (9, 21)     # api_msm.hip blsgpu_bases_precompute
SBITS = {8: 256, 4: 128, 2: 64}  # msm_plan.h msm_shape: the width the windows cover, by words per sort scalar


def recode(v, c, nwin, words=8):
    """DigitIter<words> / k_msm_digits (words = 8): the signed c-bit digits of the stored value `v` (words * 32 bits), lowest window
    first, as [(magnitude, negative)]; magnitude 0 = no entry.  words = 4 / 2: the top bit of `v` is the sign of the term, the rest
    its magnitude.  A digit above 2^(c-1) becomes its complement with a carry into the next window; the carry out of the LAST window
    is dropped -- for canonical scalars (< r < 2^255), 127-bit halves and 63-bit digits there is none, since `nwin * c` covers one
    spare bit.  A value in [r, 2^256) is recoded like any other 256-bit number: every magnitude stays <= 2^(c-1), so no index
    leaves its table, the dropped carry makes the digits stand for v - 2^(nwin c) where there is one, and the kernels report it
    through the status word."""
    bits = 32 * words
    assert 0 <= v < (1 << bits) and c >= 1
    sign = 0
    if words != 8:
        sign = v >> (bits - 1)
        v &= (1 << (bits - 1)) - 1
    nbw, mask, carry, out = 1 << (c - 1), (1 << c) - 1, 0, []
    for _ in range(nwin):
        raw = (v & mask) + carry
        v >>= c
        over = 1 if raw > nbw else 0
        out.append(((1 << c) - raw if over else raw, over ^ sign))
        carry = over
    return out


def nwin_of(c, words=8):
    return (SBITS[words] + c - 1) // c


def bucket_entries(values, c, nwin, words=8, merged=False, stride=0):
    """the bucket multiset: entry lists (index | negative << 31) per global bucket `seg * 2^(c-1) + magnitude - 1`.  Unmerged: one
    bucket set per window, index = the scalar's position; merged (resident window-shifted tables): ONE set, index = w * stride + i."""
    nbw = 1 << (c - 1)
    buckets = [[] for _ in range((1 if merged else nwin) * nbw)]
    for i, v in enumerate(values):
        for w, (mag, neg) in enumerate(recode(v, c, nwin, words)):
            if mag:
                buckets[(0 if merged else w) * nbw + mag - 1].append(((w * stride + i) if merged else i) | (neg << 31))
    return buckets


def offsets(buckets):
    """exclusive prefix of the bucket loads, nb + 1 entries: offs[nb] = the number of non-zero digits"""
    offs, run = [], 0
    for b in buckets:
        offs.append(run)
        run += len(b)
    return offs + [run]


def sort_split(c, nwin, merged=False):
    """msm_plan.h msm_sort_split: (fine_bits, ncoarse, nc) -- the key (window, |digit| - 1) is cut into a coarse part that counts in
    LDS (nc = bucket sets * ncoarse counters) and a fine part of at most 7 bits"""
    key_bits = c - 1
    coarse_bits = (key_bits - 7 if key_bits > 7 else 0) if merged else min(key_bits, 8)
    fine_bits = key_bits - coarse_bits
    assert 0 <= fine_bits <= 7
    return fine_bits, 1 << coarse_bits, (1 if merged else nwin) * (1 << coarse_bits)


def counter_tables():
    """nc for every window configuration the product accepts: {(words, c, merged): nc}"""
    t = {}
    for words in (8, 4, 2):
        for c in range(WINDOW_RANGE[0], WINDOW_RANGE[1] + 1):
            t[(words, c, False)] = sort_split(c, nwin_of(c, words))[2]
    for c in range(TABLE_WINDOW_RANGE[0], TABLE_WINDOW_RANGE[1] + 1):
        t[(8, c, True)] = sort_split(c, nwin_of(c, 8), merged=True)[2]
    return t


def item_partition(offs, cap):
    """k_item_count / k_item_fill: per bucket the (start, len) of its work items in bucket order -- `load // cap` items of `cap`
    entries, then the remainder; an empty bucket keeps one item of length 0, a load that `cap` divides has no remainder item"""
    out = []
    for b in range(len(offs) - 1):
        beg, load = offs[b], offs[b + 1] - offs[b]
        full, rem = divmod(load, cap)
        it = [(beg + j * cap, cap) for j in range(full)]
        if rem or not full:
            it.append((beg + full * cap, rem))
        out.append(it)
    return out


def item_cap(ns, c, forced=0):
    """msm_plan.h msm_shape: ~4x the mean bucket load, a power of two in [128, ITEM_CAP_MAX]"""
    if forced:
        return forced
    cap = 128
    while cap < ITEM_CAP_MAX and cap * (1 << (c - 1)) < 4 * ns:
        cap *= 2
    return cap


def level_sums(E, M, off):
    """one reduction level over the exponents E (n = len(E), a multiple of M) of one window: chunk g covers records [g M, g M + M);
    R_g = sum E_j, T_g = sum (j - g M + off) E_j.  With off = 1 at the bottom level and 0 above,
    sum_b (b + 1) E_b = sum_g T_g + M * (the same sum one level up over R)."""
    assert len(E) % M == 0
    R, T = [], []
    for g in range(len(E) // M):
        ch = E[g * M:(g + 1) * M]
        R.append(sum(ch))
        T.append(sum((j + off) * e for j, e in enumerate(ch)))
    return R, T


def window_sum(E):
    """sum_b (b + 1) E_b, and the same by the levels of api_msm.hip (fan 8, the last level M = n): the two must agree"""
    want = sum((b + 1) * e for b, e in enumerate(E))
    ts, ms, cur, off = [], [], list(E), 1
    while len(cur) > 1:
        M = 8 if len(cur) >= 8 else len(cur)
        cur, T = level_sums(cur, M, off)
        ts.append(sum(T)); ms.append(M); off = 0
    acc = 0
    for T, M in zip(reversed(ts), reversed(ms)):
        acc = T + M * acc
    # Horner: acc_l = T_l + M_l * acc_{l+1}, the top level's M multiplies nothing
    return want, (acc if ts else E[0])


# ---- the launch plan (csrc/msm_plan.h), restated from its description; tests/test_msm_plan.py compares the two ---------------------
TEAM = 8                         # team.hip.h
TEAM_LANES_MAX = 131072          # msm_plan.h
TREE_JOBS_MAX = 8                # msm.hip.h
REDUCTION_BLOCK = 256            # threads per block of the level, tree and shift-add launches


def pick_window(n, bits):
    """msm_plan.h msm_pick_window: the c in 6..16 (the smallest on a tie) that minimises n W + 2.4 W 2^(c-1), W = ceil(bits / c) -- in
    integers, five times the cost"""
    return min(range(6, 17), key=lambda c: (-(-bits // c) * (5 * n + 12 * (1 << (c - 1))), c))


def reduction_schedule(nseg, nbw):
    """msm_plan.h msm_reduction: the reduction of nseg windows of nbw bucket records each.
    levels: per level n, M = min(8, n), G = n / M, off (1 at the bottom, 0 above), form, grid, toff (records of T before this level)
    and horner (G == 1: T is the level's Horner row).  steps: after every level one pass of every unfinished T tree (a level with
    G > 1 starts one), then passes until none is left: per step (jobs of the multi launch, its grid, passes); a pass is (level, n, TM,
    TG, src, pp, horner, multi, off) with src -1 = the level's T block, else the ping-pong buffer it reads.  horner: the shifts
    log2(M_l) for l = levels - 2 .. 0."""
    levels, steps, trees = [], [], []

    def step():
        passes, jobs, teams = [], 0, 0
        for tr in trees:
            if tr["n"] <= 1:
                continue
            tm = min(8, tr["n"])
            tg = -(-tr["n"] // tm)
            multi = nseg * tg * TEAM <= TEAM_LANES_MAX and jobs < TREE_JOBS_MAX
            if multi:
                jobs += 1
                teams += nseg * tg
            passes.append((tr["level"], tr["n"], tm, tg, tr["src"], tr["pp"], tg == 1, multi, tr["off"]))
            tr["src"], tr["n"], tr["pp"] = tr["pp"], tg, tr["pp"] ^ 1
        steps.append((jobs, -(-teams * TEAM // REDUCTION_BLOCK), passes))
        return bool(passes)

    n, off, toff = nbw, 1, 0
    while n > 1:
        m = min(8, n)
        g = n // m
        if nseg * g * 2 * TEAM <= TEAM_LANES_MAX:
            form, lanes = 0, nseg * g * 2 * TEAM
        elif nseg * g * TEAM <= TEAM_LANES_MAX:
            form, lanes = 1, nseg * g * TEAM
        else:
            form, lanes = 2, nseg * g * 2
        levels.append({"n": n, "M": m, "G": g, "off": off, "form": form, "grid": -(-lanes // REDUCTION_BLOCK), "toff": toff, "horner": g == 1})
        if g > 1:
            trees.append({"level": len(levels) - 1, "n": g, "src": -1, "pp": 0, "off": toff})
        step()
        toff += nseg * g
        n, off = g, 0
    while step():
        pass
    steps.pop()                                                     # the step that found nothing to do
    return {"levels": levels, "steps": steps, "horner": [lv["M"].bit_length() - 1 for lv in reversed(levels[:-1])]}


def schedule_text(nseg, nbw):
    """the schedule in the text form of tests/cpp/msm_plan_main.cpp"""
    s = reduction_schedule(nseg, nbw)
    out = "sched nseg=%d nbw=%d levels=%d nsteps=%d :" % (nseg, nbw, len(s["levels"]), len(s["steps"]))
    for lv in s["levels"]:
        out += " L%d,%d,%d,%d,%d,%d,%d,%d" % (lv["n"], lv["M"], lv["G"], lv["off"], lv["form"], lv["grid"], lv["toff"], lv["horner"])
    out += " :"
    for jobs, grid, passes in s["steps"]:
        out += " S%d,%d" % (jobs, grid) + "".join("/%d,%d,%d,%d,%d,%d,%d,%d,%d" % p for p in passes)
    return out + " : H" + "".join(" %d" % k for k in s["horner"])


def launch_counts(group, words, c, merged=False, fast_sort=True, mont=False):
    """kernel name -> launches of ONE msm call, as kernel_timing_report() names them: group 1 / 2, words per sort scalar (8 plain, 4
    GLV halves, 2 psi digits), window c; mont: Montgomery scalars without a decomposition kernel in front"""
    nwin = nwin_of(c, words)
    s = reduction_schedule(1 if merged else nwin, 1 << (c - 1))
    k = {}

    def add(name, count=1):
        if count:
            k[name] = k.get(name, 0) + count
    if words == 8 and mont:
        add("k_scalars_from_mont")
    if words != 8:
        add("k_glv_decompose" if words == 4 else "k_gls_decompose")
    if fast_sort:
        for name in ("k_sort_hist<%d>" % words, "k_sort_scan", "k_sort_scatter<%d>" % words, "k_sort_fine"):
            add(name)
    else:
        for name in ("k_msm_digits", "k_scan_block_sums", "k_scan_top", "k_scan_apply", "k_msm_scatter"):
            add(name)
    for name in ("k_item_count", "k_item_scan", "k_item_fill", "k_msm_accumulate<F>" if group == 1 else "k_msm_accumulate_g2pair", "k_msm_heavy<F>"):
        add(name)
    pair = "k_wsum_level_pair" if group == 1 else "k_wsum_level_g2pair"
    for lv in s["levels"]:
        add(("k_wsum_level_team2<F>", "k_wsum_level_team<F>", pair)[lv["form"]])
    for jobs, _, passes in s["steps"]:
        add("k_tree_sum_team_multi<F>", 1 if jobs else 0)
        add("k_tree_sum<F>", sum(1 for p in passes if not p[7]))
    add("k_shift_add_team<F>", len(s["horner"]))
    add("k_msm_combine_team<F>")
    add("k_proj_export<F>")
    return k


# ---- scalars with prescribed digits (tests/test_msm_pipeline_gpu.py) -----------------------------------------------------------
def digit_values(c):
    """every signed digit the recoding can produce: -(2^(c-1) - 1) .. -1, 1 .. 2^(c-1), 0 -- 2^c values"""
    nbw = 1 << (c - 1)
    return list(range(-(nbw - 1), 0)) + list(range(1, nbw + 1)) + [0]


def covering_values(c, usable_bits, rng, signed=False):
    """2^c integers of magnitude below 2^usable_bits whose signed c-bit digits, in every window that lies wholly below `usable_bits`
    (nfull = usable_bits // c of them), run through ALL 2^c digit values exactly once: D_w(i) = vals[(a_w i + b_w) mod 2^c] with
    a_w odd.  Signed digits in (-2^(c-1), 2^(c-1)] represent an integer uniquely, so the recoding of the value returns exactly
    these digits.  signed = False: a digit +1 in the next window keeps every value positive (c must not divide usable_bits: the
    closing digit has to fit).  signed = True (the halves of a split, which carry a sign of their own): no closing digit, the value
    takes the sign of its top non-zero digit.  The recoding of |v| under the flipped term sign yields the very same entries as long
    as no digit of a negative v is +2^(c-1) (its negative is outside the digit set), so a_w, b_w are redrawn until the index that
    takes +2^(c-1) in window w has a positive top digit.
    Returns (values, nfull)."""
    vals = digit_values(c)
    n = 1 << c
    nbw = n >> 1
    nfull = usable_bits // c
    assert nfull >= 1 and (signed or c * nfull < usable_bits)
    ab = [None] * nfull
    for w in reversed(range(nfull)):
        while True:
            a, b = (rng.next() | 1) % n, rng.next() % n
            ab[w] = (a, b)
            if not signed or w == nfull - 1:
                break
            i_top = (vals.index(nbw) - b) * pow(a, -1, n) % n       # the index whose digit in window w is +2^(c-1)
            if vals[(ab[-1][0] * i_top + ab[-1][1]) % n] > 0:
                break
    out = []
    for i in range(n):
        v = 0 if signed else 1 << (c * nfull)
        for w, (a, b) in enumerate(ab):
            v += vals[(a * i + b) % n] << (c * w)
        assert abs(v) < (1 << usable_bits) and (signed or v > 0)
        out.append(v)
    return out, nfull


def coverage(digit_lists, c, nfull, sign=0):
    """True when, in each of the first nfull windows, the recoded digits (the lists `recode` returns, one per scalar, all of terms
    with the sign bit `sign`) hit every (magnitude, negative) entry a window has -- magnitudes 1 .. 2^(c-1) - 1 with both signs,
    2^(c-1) as a positive digit only -- exactly once, and the zero digit once"""
    nbw = 1 << (c - 1)
    want = sorted([(m, sign) for m in range(1, nbw + 1)] + [(m, sign ^ 1) for m in range(1, nbw)] + [(0, 0)])
    for w in range(nfull):
        if sorted((d[w][0], d[w][1] if d[w][0] else 0) for d in digit_lists) != want:
            return False
    return True
