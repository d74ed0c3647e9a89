"""Every stage of the C ABI on contexts made for the test: as a context's first work, across table growth in both
directions, with tables grown by another stage, across evictions of the two caches, across wraps of the mailbox ring
and of the staging arena, with the timers on and after refused calls.

A ``Context`` keeps state between calls (csrc/context.cpp, csrc/ntt.hip, csrc/quotient.hip):

* ``M``   Montgomery twiddles, one log (``ensure_twiddles``), grown on demand, never shrunk;
* ``Pf``  Plantard forward twiddles and ``Pi`` Plantard inverse twiddles, a log each (``ensure_plant_twiddles``);
* the LDE scale tables keyed by (log_n, shift), none for shift 1, 8 entries, least recently used evicted;
* the selector tables keyed by (log_n, log_qd, shift), 2 entries, least recently used evicted;
* the mailbox ring (16384 words, slots of 16), the staging arena (1 MiB, 64-byte granules), the pinned buffer, the
  ticket words and a commitment's column-table flag, all made on first use.

What a call asks for (read from the call sites): ``dft(n)`` M, Pf, Pi >= n; ``lde(n, +b)`` and a commit of blowup b M,
Pf >= n + b and Pi >= n; ``fold(h)`` M >= h + 1; a FRI round of h leaves after a fold M >= h + 2; the quotient of
degree 2^q M >= n + q; the open calls M >= n + b.  A log of 0 is asked for as 1.  The shared context of the other GPU
modules has served hundreds of calls when a test reaches it, so a missing or short ``ensure_*``, a cache hit that
ignores a key component or a pointer kept across a growth cannot show there.  Here the state before every checked
call follows from the calls before it on the same context and is written in each scenario's docstring as (M, Pf, Pi)
or as the cache contents; ``-`` is a table that does not exist yet.

Every comparison is exact and against the CPU oracle (tests/_context_cases.py); every context is ``ts.Context(0)``
made inside the test and closed before it returns; at most two are alive at once; one process."""
import threading

import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd._lib import TsError

import _context_cases as cc
import _derive_cases as dc
import _iterate_cases as ic
import _join_cases as jc
from _context_cases import fresh_context
from _field_cases import EXTREME_KINDS, P
from test_gpu_dft import rand_mat, rand_shift

pytestmark = pytest.mark.gpu
TS_ERR_INVALID, TS_ERR_INVARIANT = 1, 5


@pytest.fixture(scope="module", autouse=True)
def built():
    from tapstark_amd.build import build

    build()


@pytest.fixture(autouse=True)
def interpreter(monkeypatch):
    """Every AIR of this module runs on the interpreter: the same words, no background compile to wait for."""
    monkeypatch.setenv("TS_NO_JIT", "1")


# ------------------------------------------------------------------ A. first work of a context
FIRST = [("dft", n, {"first": f}) for n in (0, 13) for f in cc.DFT_CALLS] + \
        [("lde", n, kw) for n in (0, 13) for kw in ({"added_bits": 1, "shift": 31}, {"added_bits": 2, "shift": rand_shift(9)},
                                                     {"added_bits": 1, "shift": 1})] + \
        [("commit", 0, {}), ("commit", 13, {}), ("commit", 13, {"log_blowup": 2, "shift": 31 * pow(cc.G27, 1 << 12, P) % P}),
         ("quotient", 1, {"qd": 1}), ("quotient", 1, {"qd": 2}), ("quotient", 13, {"qd": 1}), ("quotient", 13, {"qd": 2}),
         ("open", 1, {"qd": 1}), ("open", 13, {"qd": 2}), ("fold", 0, {}), ("fold", 13, {}), ("fri", 1, {}), ("fri", 13, {}),
         ("domain", 1, {}), ("domain", 13, {}), ("multi", 6, {}), ("prove", 0, {}), ("prove", 13, {})]


@pytest.mark.parametrize("probe,log_n,kw", FIRST,
                         ids=[f"{p}-2^{n}" + "".join(f"-{v}" for v in kw.values()) for p, n, kw in FIRST])
def test_a_first_work_of_a_context(orc, probe, log_n, kw):
    """State before the one checked probe: (-, -, -), both caches empty, no ring, no arena, no pinned buffer, no
    ticket words.  The probe's first launch is the context's first device work, at the smallest height that touches
    a table (a log of 0 or 1) and at 2^13, the first two-pass NTT plan.  ``fold`` and ``fri`` ask for M = log_h + 1
    and log_h + 2, which nothing before them has built.  ``commit`` and ``prove`` are the context's first commit: the
    ticket words are made and zeroed, and the column-table flag starts false.
    Guards: a call site that reads ``d_twiddle_*`` / ``d_plant_*`` without its ``ensure_*`` (ntt_dft.hip:174-175,
    ntt_lde.hip:455 and :560-561, fri.hip:65, :141, :169 and :408, quotient.hip:93, open.hip:59, :268, :393 and :422,
    open_multi.hip:52, prover.cpp:229 and :459, prove_multi.cpp:332) and ``Context::ticket`` (context.cpp:136)."""
    with fresh_context() as ctx:
        cc.PROBES[probe](ctx, orc, log_n, **kw)


# ------------------------------------------------------------------ B. growth ladder
LADDER = (1, 5, 12, 13, 15, 18, 19)
EXTREME_AT = (15, 18, 19)


def ladder_widths(log_n):
    return (1,) if log_n >= 18 else (1, 3)


def extreme_cases(log_n):
    """(kind, width): every kind at 2^15 x 3; at width 1 ``alt_cols`` is ``zero``, so three kinds."""
    return [(k, 1) for k in EXTREME_KINDS if k != "alt_cols"] if log_n >= 18 else [(k, 3) for k in EXTREME_KINDS]


def ladder_step(ctx, orc, probe, log_n, refs, extremes):
    seeded = rand_shift(500 + log_n)
    for w in ladder_widths(log_n):
        if probe == "dft":
            cc.dft(ctx, orc, log_n, w=w, refs=refs)
        elif probe == "lde":
            for shift in (31, seeded):
                cc.lde(ctx, orc, log_n, 1, shift, w=w, refs=refs)
        elif probe == "commit":
            cc.commit(ctx, orc, log_n, w=w, refs=refs)
    if probe == "quotient":  # the AIR fixes the width: Fibonacci (2 columns), and SynthMulAir(7) up to 2^15
        cc.quotient(ctx, orc, log_n, qd=1, refs=refs)
        if log_n <= 15:
            cc.quotient(ctx, orc, log_n, qd=2, refs=refs)
    if extremes and log_n in EXTREME_AT and probe != "quotient":
        for kind, w in extreme_cases(log_n):
            if probe == "dft":
                cc.dft(ctx, orc, log_n, w=w, kind=kind)
            elif probe == "lde":
                cc.lde(ctx, orc, log_n, 1, seeded, w=w, kind=kind)
            else:
                cc.commit(ctx, orc, log_n, w=w, kind=kind)


@pytest.mark.parametrize("probe", ["dft", "lde", "commit", "quotient"])
def test_b_growth_ladder_up_then_down(orc, probe):
    """One context per probe; log_n = 1, 5, 12, 13, 15, 18, 19 ascending, then the same descending; widths 1 and 3
    (1 only at 2^18 and 2^19); added_bits / log_blowup 1; ``lde`` with shifts 31 and one seeded per height.

    State before the call at log_n, ascending (n' = the height before, 0 at the start):

    ========  ====================  ==========================================================
    probe     (M, Pf, Pi) before    the call asks for
    ========  ====================  ==========================================================
    dft       (n', n', n')          (n, n, n): all three too small
    lde       (n'+1, n'+1, n')      (n+1, n+1, n): all three too small
    commit    (n'+1, n'+1, n')      (n+1, n+1, n)
    quotient  (n'+1, n'+1, n')      its commit (n+1, n+1, n), then M >= n + q: already there
    ========  ====================  ==========================================================

    Descending, the state stays at the top -- (19, 19, 19) for dft, (20, 20, 19) for the others -- and every call
    reads a prefix of tables built for 2^19 or 2^20: a kernel that strides a table by its own n, not by the table's
    size, is right only there.  Plan rows 15, 18 and 19 (strided passes of 3, 6 and 7 stages, ntt_plan.hpp) are
    compared bit for bit here, on seeded and -- ascending -- on the extreme matrices, for dft, idft, the coset forms,
    coset_lde and commit.  The scale-table cache sees 14 distinct (log_n, shift) keys in the ``lde`` ladder: those
    of 2^1, 2^5 and 2^12 are evicted during the ascent and rebuilt on the descent.
    Guards: the ``want <= have`` tests of ``ensure_twiddles`` / ``ensure_plant_twiddles`` (context.cpp:238 and :257),
    the table strides of ``twiddles_fwd`` / ``twiddles_inv`` and the lazy [0, 2p) words between the strided and the
    contiguous pass (ntt_rounds.hpp ``tile_forward_rt`` / ``tile_inverse_rt``)."""
    refs = {}
    with fresh_context() as ctx:
        for log_n in LADDER:
            ladder_step(ctx, orc, probe, log_n, refs, extremes=True)
        for log_n in reversed(LADDER):
            ladder_step(ctx, orc, probe, log_n, refs, extremes=False)


# ------------------------------------------------------------------ C. tables grown by another stage
def test_c_tables_grown_by_another_stage(orc):
    """One context, a fixed interleaving.  (M, Pf, Pi) AFTER each call; the state before a call is the line above.

    ====  =========================  ============  ==================================================================
    step  call                       state after   what the call finds
    ====  =========================  ============  ==================================================================
    1     fold, log_h 11             (12, -, -)    M absent
    2     lde(6, +1), shift 31       (12, 7, 6)    M larger than its 7; Pf and Pi absent
    3     dft(10)                    (12, 10, 10)  M larger; Pf and Pi too small
    4     lde(9, +4), seeded shift   (13, 13, 10)  M and Pf too small by 1 and 3; Pi (needs 9) larger
    5     idft(10)                   (13, 13, 10)  Pi exact; M and Pf larger
    6     lde(13, +1), shift 31      (14, 14, 13)  all three too small: a two-pass plan on tables grown by this call
    7     dft(3)                     (14, 14, 13)  all three larger
    8     fold, log_h 14             (15, 14, 13)  M too small while Pf and Pi are larger than anything asked so far
    9     lde(12, +2), seeded shift  (15, 14, 13)  Pf exact (14); M and Pi larger
    10    fold, log_h 13             (15, 14, 13)  M larger: the fold reads Winv[2^13, 2^14) of a 2^15-word table
    11    quotient(5, degree 2)      (15, 14, 13)  everything larger; then open(7): the same
    ====  =========================  ============  ==================================================================

    Absent / too small, exact and larger-while-another-grows, per table: M 1 | 4, 6 (grown to exactly 13, 14) and 8 |
    2, 3 and 10; Pf 2 | 9 | 5, 7 with step 8 growing M; Pi 2 | 5 | 4, where M and Pf grow.  (The transforms multiply by
    the Plantard tables only; the Montgomery tables are read by the fold, the FRI rounds, the selectors and the
    open kernels, hence steps 1, 8, 10 and 11.)
    Guards: ``ensure_lde_twiddles`` growing Pf but not Pi (context.hpp:189-191) with ntt_lde.hip:561 asking for Pi on
    its own; a grow of one table leaving the pointers of the other two valid (context.cpp:241-246 and :260-266 free
    only their own)."""
    with fresh_context() as ctx:
        d = ts.Radix2Dft(ctx)
        cc.fold(ctx, orc, 11)
        cc.lde(ctx, orc, 6, 1, 31)
        cc.dft(ctx, orc, 10)
        cc.lde(ctx, orc, 9, 4, rand_shift(94))
        x = cc.matrix(10, 3)
        cc.equal(d.idft_batch(x).download(), orc.dft_batch(x, inverse=True), "step 5: idft(10)")
        cc.lde(ctx, orc, 13, 1, 31)
        cc.dft(ctx, orc, 3)
        cc.fold(ctx, orc, 14)
        cc.lde(ctx, orc, 12, 2, rand_shift(122))
        cc.fold(ctx, orc, 13)
        cc.quotient(ctx, orc, 5, qd=2)
        cc.open_(ctx, orc, 7)


# ------------------------------------------------------------------ D. scale-table cache
D_CFG = (1, 3, 0)


def test_d_scale_table_cache(orc):
    """Sized for 8 entries: ``ctx.scale_tables.size() >= 8`` in ``coset_scale_table`` (csrc/ntt.hip).  Width 2,
    added_bits 1; s0 .. s9 are ten seeded shifts, none 1.  The sequence runs at log_n = 6, then again at 13 on the
    same context, so that the second pass starts on a cache full of keys of the other height.  Cache contents, least
    recently used first, before each call of a pass that starts on an empty cache (the second pass evicts the first
    pass's keys one by one and reaches the same contents at call 9):

    =====  =========  ======================================  ===============================
    call   shift      cache before                            the lookup
    =====  =========  ======================================  ===============================
    1-8    s0 .. s7   s0 .. s(k-1)                            miss, a table is added
    -      1          (unchanged)                             no table: the constant 1/n
    9      s8         s0 s1 s2 s3 s4 s5 s6 s7                 miss, s0 evicted
    10     s9         s1 s2 s3 s4 s5 s6 s7 s8                 miss, s1 evicted
    -      1          (unchanged)
    11     s0         s2 s3 s4 s5 s6 s7 s8 s9                 miss: rebuilt after its eviction, s2 evicted
    12     s9         s3 s4 s5 s6 s7 s8 s9 s0                 hit
    =====  =========  ======================================  ===============================

    Every probe asks twice (natural, then bit-reversed rows): the second lookup is a hit on the newest entry.  Then
    one shift at both heights back to back, (13, t) (6, t) and (6, u) (13, u): a lookup that ignored log_n would hand
    a 2^13-word table to the 2^6 call or read 2^13 words of a 2^6-word one.  Then, on this cache of 8 entries, the
    launch of two matrices at once (``coset_lde`` with ``evals2`` / ``shift2``, prover_common.cpp "exactly two
    column-major matrices"):

    * ``commit_pair`` at 2^6, 2^13 and 2^6 again: two quotient chunks committed on two seeded domains, so BOTH
      lookups of the pair launch miss on a full cache and evict, and the table of the first lookup must outlive the
      second (it carries the newest clock when the second picks its victim);
    * SynthMulAir(7) proofs, FRI (1, 3, 0), at log_n 3, 4, 5, 6, 7, 6, 5, 4, 3, each byte-equal to the oracle's.  A
      proof brings two keys of its height alone: (log_n, 31) with its trace commit and (log_n, 1 / g) as ``shift2``
      of its pair launch, g the generator of order 2^(log_n + 1); the ``shift`` of that launch is 1, the chunk whose
      domain is the LDE's first coset, which has no table.  Five heights: ten keys, so the descent finds the keys
      of 2^3, 2^4 and 2^5 evicted.

    Guards: the key test ``t.log_n == log_n && t.shift == shift`` and the victim choice (ntt.hip:112-129); the order
    of the two lookups at ntt_lde.hip:567-568."""
    shifts = [rand_shift(2000 + k) for k in range(10)]
    assert len(set(shifts)) == 10 and 1 not in shifts and 31 not in shifts
    refs = {}
    with fresh_context() as ctx:
        for log_n in (6, 13):
            def run(shift):
                cc.lde(ctx, orc, log_n, 1, shift, w=2, refs=refs)
            for k in range(8):
                run(shifts[k])
                if k in (0, 4):
                    run(1)
            run(1)
            run(shifts[8])
            run(shifts[9])
            run(1)
            run(shifts[0])
            run(shifts[9])
        t, u = rand_shift(2100), rand_shift(2101)
        cc.lde(ctx, orc, 13, 1, t, w=2)
        cc.lde(ctx, orc, 6, 1, t, w=2)
        cc.lde(ctx, orc, 6, 1, 1, w=2)
        cc.lde(ctx, orc, 6, 1, u, w=2)
        cc.lde(ctx, orc, 13, 1, u, w=2)
        pair = [rand_shift(2200 + k) for k in range(6)]
        cc.commit_pair(ctx, orc, 6, pair[0:2])
        cc.commit_pair(ctx, orc, 13, pair[2:4])
        cc.commit_pair(ctx, orc, 6, pair[4:6])
        for log_n in (3, 4, 5, 6, 7, 6, 5, 4, 3):
            cc.prove(ctx, orc, log_n, qds=(2,), cfg=D_CFG, refs=refs)


# ------------------------------------------------------------------ E. selector-table cache
def test_e_selector_table_cache(orc):
    """Sized for 2 entries: ``Context::sel_tables`` (csrc/context.hpp) as ``selector_table`` (csrc/quotient.hip) uses
    it.  Shapes that differ in exactly one key component: A = (5, degree 1), B = (5, degree 2), C = (6, degree 1); the
    shift is the prover's 31 in all of them.  Cache contents, least recently used first, before each call:

    ====  =====  ============  ====================================
    call  shape  cache before  the lookup
    ====  =====  ============  ====================================
    1     A      -             miss
    2     B      A             miss
    3     C      A B           miss, A evicted
    4     A      B C           miss, B evicted
    5     B      C A           miss, C evicted
    6     C      A B           miss, A evicted
    7     A      B C           miss, B evicted
    8     A      C A           hit
    9     B      C A           miss, C evicted
    10    A      A B           hit
    11    B      B A           hit: two live entries alternating
    ====  =====  ============  ====================================

    Guards: the three-part key test of quotient.hip:109 (a lookup that ignored log_qd would give B the selectors of A,
    half as many words; one that ignored log_n would give C those of A) and the sync before the free at :113."""
    shapes = {"A": (5, 1), "B": (5, 2), "C": (6, 1)}
    refs = {}
    with fresh_context() as ctx:
        for name in "ABCABC" + "AA" + "BAB":
            log_n, qd = shapes[name]
            cc.quotient(ctx, orc, log_n, qd=qd, refs=refs)


def test_e_selector_shift_is_part_of_the_key(orc):
    """The third key component.  One ``LocalCommGroup(2)``; each rank's own context alternates
    ``prove_sharded(local_quotient=True)`` -- the quotient on the rank's own cosets, with the shift s_g = 31
    w_N^bitrev(beta0) of its first coset (csrc/sharded.cpp) -- and a plain ``prove`` of the same 2^6 shape (log_n 6,
    log_qd 1, shift 31), three times.  Rank 0 owns coset 0, so its s_g is 31 and every call after its first is a hit
    on one entry.  Rank 1's s_g differs from 31; its cache before its calls: - | (6, 1, s_1) | (6, 1, s_1) (6, 1, 31)
    | ...: from the third call on both keys are live and every call must hit the entry of ITS shift, beside an
    entry that differs in the shift alone.  Every proof is byte-equal to the oracle's.  Sized for the 2 entries of
    ``Context::sel_tables`` (csrc/context.hpp).
    Guards: ``t.shift == shift`` in quotient.hip:109."""
    from tapstark_amd.comm import LocalCommGroup

    G, log_n, cfg = 2, 6, (2, 3, 0)
    air, trace, pis, tape = cc.statement(2, log_n)
    want = orc.prove(orc.FriConfig(*cfg), tape, trace, pis)
    n = 1 << log_n
    group = LocalCommGroup(G)
    res, errs = [[] for _ in range(G)], [None] * G

    def rank(r):
        try:
            with fresh_context() as c:
                conf = ts.StarkConfig(ts.TwoAdicFriPcs(ts.FriConfig(*cfg), c))
                cair = ts.CompiledAir(c, tape)
                rows = np.ascontiguousarray(trace[r * n // G:(r + 1) * n // G])
                for _ in range(3):
                    p = ts.prove_sharded(conf, cair, ts.BfChallenger(), rows.copy(), pis, group.comm(r),
                                         local_quotient=True)
                    res[r].append(p.words)
                    res[r].append(ts.prove(conf, cair, ts.BfChallenger(), trace.copy(), pis).words)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    th = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank is stuck in a collective"
    for r in range(G):
        assert errs[r] is None, f"rank {r}: {errs[r]!r}"
        assert len(res[r]) == 6
        for k, words in enumerate(res[r]):
            cc.equal(words, want, f"rank {r}, proof {k} ({'plain' if k % 2 else 'sharded'})")


# ------------------------------------------------------------------ F. rings and staging
F_CFG = (2, 3, 4)


def test_f_mailbox_boundary_and_wrap(orc):
    """Sized for the 16384-word ring of ``Context::mailbox`` (csrc/context.cpp: ``WORDS``; a message above WORDS / 4 =
    4096 words takes the separate buffer).  prover.cpp asks for ``4 * raw.size()`` words for the opened values,
    ``raw.size()`` = 2 w + 4 qd EF4 elements: 8 w + 16 qd words, 4096 at w = 508 with SynthMulAir's two chunks -- the
    largest message of the ring -- and 4104 at w = 509, the first of the separate buffer.  Each of the two commits of
    a proof takes a slot of 16 words for its root first.  2^3 rows, FRI (2, 3, 4).

    First each width on a context of its own (no ring / no separate buffer yet).  Then one context; ring offset
    before and after the opened-value message of each proof:

    =====  =====  =======================  ==============================================
    proof  width  ring offset              separate buffer
    =====  =====  =======================  ==============================================
    1      508    32 -> 4128               -
    2      509    4160 (unchanged)         made, 4104 words
    3      508    4192 -> 8288             kept
    4      7      8320 -> 8416 (96 words)
    5      508    8448 -> 12544
    6      508    12576 -> WRAP 0 -> 4096  (12576 + 4096 > 16384)
    7      509    4128 (unchanged)         reused after ring use
    8      7      4160 -> 4256
    =====  =====  =======================  ==============================================

    Guards: ``words > WORDS / 4`` and the wrap test of context.cpp:186 and :201 (a `>=` in the first sends 4096 words
    to a buffer of its own; a ring slot that runs past the end is host memory the kernels write)."""
    refs = {}
    for width in (508, 509):
        with fresh_context() as ctx:
            cc.prove_mul(ctx, orc, 3, width, F_CFG, refs=refs)
    with fresh_context() as ctx:
        for width in (508, 509, 508, 7, 508, 508, 509, 7):
            cc.prove_mul(ctx, orc, 3, width, F_CFG, refs=refs)


def u8_upload(ctx, width, seed, keep):
    """An asynchronous packed upload of one row of ``width`` u8 columns: its column table (8 bytes a column) is what
    ``launch_ingest`` stages.  Returns (matrix, expected words); ``keep`` holds the pinned source."""
    from test_gpu_ingest import U8, expected

    words = np.random.default_rng(seed).integers(0, 256, size=(1, width), dtype=np.uint32)
    words[0, 0], words[0, -1] = 255, 0
    fmt = ts.TraceFormat(U8)
    assert fmt.nbytes(1, width) == width
    pinned = ts.PinnedHostBytes(width)
    pinned.array[:] = words.reshape(-1).astype(np.uint8)  # one byte a column, columns back to back: the u8 rows form
    keep.append(pinned)
    return ts.DeviceMatrix.upload_packed_async(ctx, pinned, fmt, 1, width), expected(words, [U8])


def test_f_staging_arena(orc):
    """Sized for the 1 MiB arena of ``Context::stage`` (csrc/context.cpp) and the 1 MiB bypass of ``h2d``
    (csrc/prover_common.cpp) and ``launch_ingest`` (csrc/ingest.hip).  Uploads through the arena: the column table of
    a packed upload (8 bytes a column: any size to the byte), the program image of derive and iterate, the
    challenge-power lists of a proof.  Nothing waits between the calls of a group; the results are downloaded and
    compared at its end, so a slot that was overwritten before its copy ran shows as wrong words.

    =====  ==============================  ===========================  =====================================
    step   upload (bytes -> granules)      arena (size, offset) before  what happens
    =====  ==============================  ===========================  =====================================
    1      5 columns (40 -> 64)            none                         (i) made: 1 MiB, offset 64
    2      derive and iterate images       1 MiB, 64                    (i) small, offset a few KiB
    3      65537 columns (524296 ->        1 MiB, a few KiB             (ii) more than half: wait, 2 MiB made,
           524352)                                                      offset 524352
    4      131072 columns (1048576)        2 MiB, 524352                (iv) exactly half: kept, offset 1572928
    5      131072 columns (1048576)        2 MiB, 1572928               (iii) past the end: wait, offset 0 ->
                                                                        1048576
    6      131073 columns (1048584)        2 MiB, 1048576               (v) above 1 MiB: not staged
    7      derive image, a proof           2 MiB, 1048576               small, behind step 5's slot
    =====  ==============================  ===========================  =====================================

    Guards: ``need > h_arena_bytes / 2`` and the wrap with its ``sync()`` (context.cpp:146-159), the ``<= 1 MiB`` tests
    of prover_common.cpp:19 and ingest.hip:208."""
    keep, pending = [], []
    with fresh_context() as ctx:
        def flush():
            for what, m, want in pending:
                cc.equal(m.download(), want, what)
            pending.clear()

        pending.append(("step 1: 5 columns", *u8_upload(ctx, 5, 1, keep)))
        rows = dc.random_rows(3, 64, 4)
        dprog = dc.random_program(3, 4)
        pending.append(("step 2: derive", ts.DeviceMatrix.upload(ctx, rows).derive(dprog), dc.reference(dprog, rows)))
        irows = ic.with_resets(dc.random_rows(4, 64, 3), 0, ic.starts_of_lengths([4] * 16)[0], 4)
        iprog = ic.sponge_like(3, 0)
        pending.append(("step 2: iterate", ts.DeviceMatrix.upload(ctx, irows).iterate(iprog), ic.reference(iprog, irows)))
        pending.append(("step 3: 65537 columns", *u8_upload(ctx, 65537, 3, keep)))
        flush()
        pending.append(("step 4: 131072 columns", *u8_upload(ctx, 131072, 4, keep)))
        pending.append(("step 5: 131072 columns", *u8_upload(ctx, 131072, 5, keep)))
        pending.append(("step 6: 131073 columns", *u8_upload(ctx, 131073, 6, keep)))
        src = ts.DeviceMatrix.upload(ctx, rows)
        pending.append(("step 7: derive", src.derive(dprog), dc.reference(dprog, rows)))
        flush()
        cc.prove(ctx, orc, 5)


def test_f_pinned_staging_and_downloads(orc):
    """Downloads of 2^6, 2^18, 2^6, 2^20 and 2^10 words from one context, each equal to what was uploaded.  Today
    ``ts_matrix_download`` copies into the caller's buffer and waits (csrc/abi.cpp); ``Context::pinned``
    (csrc/context.cpp: one page-locked buffer, 64 KiB doubling, waited for and freed when it grows) has no caller.
    The sizes cross its 64 KiB start twice and come back below it, so a download path that is moved onto it -- a
    buffer freed while a copy still writes it, a smaller request reading a stale prefix -- shows here."""
    with fresh_context() as ctx:
        for k, log_words in enumerate((6, 18, 6, 20, 10)):
            x = rand_mat(300 + k, 1 << log_words, 1)
            cc.equal(ts.DeviceMatrix.upload(ctx, x).download(), x, f"download of 2^{log_words} words")


# ------------------------------------------------------------------ G. timers on
def test_g_timers_on_from_the_first_call(orc):
    """``set_kernel_timing(True)`` and ``set_timing(True)`` before any device work: every launch is bracketed by
    events and every stage by a timer while the tables are first built.  State before: (-, -, -); after lde(13, +1)
    (14, 14, 13); the commit at 2^13 and the proofs at 2^5 find everything larger.  The timings are taken and
    discarded; the results are the oracle's."""
    with fresh_context() as ctx:
        ctx.set_kernel_timing(True)
        ctx.set_timing(True)
        cc.lde(ctx, orc, 13, 1, 31)
        cc.commit(ctx, orc, 13)
        cc.prove(ctx, orc, 5)
        assert ctx.take_kernel_timings(), "kernel timing was on: launches were recorded"
        ctx.take_timings()
        ctx.set_kernel_timing(False)
        ctx.set_timing(False)


# ------------------------------------------------------------------ H. after a refusal
def test_h_after_a_refusal(orc):
    """One context; after each refusal the next lde(13, +1) and proofs (2^5) are exact.

    ====  ==============================================================  =====================================
    step  refused call                                                    state it leaves
    ====  ==============================================================  =====================================
    1     coset_lde_batch with shift 0: TS_ERR_INVALID before any launch  (-, -, -): the lde after it builds all
    2     join with a missing key and no count asked: TS_ERR_INVARIANT    (14, 14, 13); the join's kernels ran
          after its launches                                              and its blocks went back to the pool
    3     iterate with an over-long group: TS_ERR_INVARIANT after its     the same
          counting launches
    4     LogUp build with a zero denominator: TS_ERR_INVARIANT           the same
    ====  ==============================================================  =====================================

    Guards: the error paths giving their pool blocks back while the stream may still use them, and leaving no sticky
    HIP error for the next launch check (``guard`` in csrc/abi.cpp)."""
    from tapstark_amd.air import LogUp
    from test_gpu_aux import SPECS, _challenges, _logup_trace
    from test_gpu_iterate import grouped

    refs = {}

    def still_exact(ctx):
        cc.lde(ctx, orc, 13, 1, 31, refs=refs)
        cc.prove(ctx, orc, 5, refs=refs)

    with fresh_context() as ctx:
        dm = ts.DeviceMatrix.upload(ctx, cc.matrix(13, 3))
        with pytest.raises(TsError) as e:
            ts.Radix2Dft(ctx).coset_lde_batch(dm, 1, 0)
        assert e.value.code == TS_ERR_INVALID and "shift" in str(e.value)
        still_exact(ctx)

        spec, src, table = jc.case(3, 64, 8, 1, 1, hit=0.5)
        assert jc.reference(spec, src, table)[1] > 0, "the case has a miss"
        with pytest.raises(TsError) as e:
            ts.DeviceMatrix.upload(ctx, src).join_rows(ts.DeviceMatrix.upload(ctx, table), spec)
        assert e.value.code == TS_ERR_INVARIANT and "is in no table row" in str(e.value)
        still_exact(ctx)

        rows = grouped(3, 3, [40] * 25 + [24] + [40] * 24 + [64])
        with pytest.raises(TsError) as e:
            ts.DeviceMatrix.upload(ctx, rows).iterate(ic.sponge_like(3, 0, max_group_rows=40))
        assert e.value.code == TS_ERR_INVARIANT and "row 1984 has 64 rows" in str(e.value)
        still_exact(ctx)

        n = 128
        trace = _logup_trace(n)
        trace[:, 0] = 1000 + 3 * np.arange(n)
        ch = _challenges(4)
        ch[:4] = (P - int(trace[37, 0]), 0, 0, 0)
        with pytest.raises(TsError) as e:
            LogUp(SPECS[2]).build(ts.DeviceMatrix.upload(ctx, trace), ch)
        assert e.value.code == TS_ERR_INVARIANT and "row 37, interaction 0" in str(e.value)
        still_exact(ctx)
