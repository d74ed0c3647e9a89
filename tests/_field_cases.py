"""Operands and exact expectations for the field probe (tap-stark_amd/probe/field_probe.hip), shared by
tests/test_field_cpu.py (host build of csrc/bb.hpp, no GPU) and tests/test_gpu_field.py (device build).

Every expectation is plain Python `int` arithmetic on the definitions: R = 2^32, Montgomery form of x is
x R mod p, EF4 = F[x]/(x^4 - 11).  Nothing here is computed by the code under test, and no operand is skipped:
where an operation has no mathematical value (the inverse of 0) the expected word is stated.

Operands: the edge set E of the field (0, 1, 2, p-2, p-1, the halves, R mod p and its negative, 2^k, p - 2^k,
2^k - 1) together with e R^-1 for every member, so that the Montgomery FORM of an operand hits the same edges;
E x E for two-operand operations plus 2^16 seeded pairs; {p, p+1, 2p-2, 2p-1} on top for the operations that
take the lazy range [0, 2p); the exact bounds of the bb.hpp comments for the 64-bit accumulators.
"""
import os
import subprocess

import numpy as np

P = 0x78000001
R = 1 << 32
RINV = pow(R, -1, P)
R_MOD_P = R % P
G27 = 0x1A427A41
MAGIC = 0x42465042
PROBE_TIMEOUT_S = 120

OPS = {"consts": 0, "add": 1, "sub": 2, "neg": 3, "red2p": 4, "mont_reduce": 5, "mont_mul": 6, "to_mont": 7,
       "from_mont": 8, "mul": 9, "mont_inv": 10, "inv_canon": 11, "mont_mul_lazy": 12, "lazy": 13,
       "lazy_cadence3": 13, "ef_add": 14, "ef_sub": 15, "ef_neg": 16, "ef_mul": 17, "ef_mul_base": 18,
       "ef_inv_parts": 19, "ef_inv": 20, "ef_pow": 21, "bitrev32": 22, "two_adic_generator": 23, "pow_canon": 24,
       "mont_pow": 25, "bfly_fwd": 32, "bfly_inv": 33, "bfly_fwd_top": 34, "bfly_inv_top": 35}
DEVICE_ONLY = ("bfly_fwd", "bfly_inv", "bfly_fwd_top", "bfly_inv_top")


def probe_path():
    from tapstark_amd.build import LIBDIR, build

    build()
    return os.path.join(LIBDIR, "field_probe")


# ------------------------------------------------------------------------------------------------ operands
def edge_set():
    e = {0, 1, 2, P - 2, P - 1, (P - 1) // 2, (P + 1) // 2, R_MOD_P, P - R_MOD_P}
    for k in range(31):
        e |= {1 << k, P - (1 << k), (1 << k) - 1}
    e |= {x * RINV % P for x in e}
    return sorted(e)


E = edge_set()
LAZY = sorted(set(E) | {P, P + 1, 2 * P - 2, 2 * P - 1})


def _pairs(left, right, seed, hi_left, hi_right, n_random=1 << 16):
    """left x right, then n_random seeded pairs below (hi_left, hi_right)."""
    grid = np.array([(a, b) for a in left for b in right], dtype=np.uint64)
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.integers(0, hi_left, n_random, dtype=np.uint64),
                    rng.integers(0, hi_right, n_random, dtype=np.uint64)], axis=1)
    return np.concatenate([grid, rnd]).astype(np.uint32)


def _singles(values, seed, hi, n_random=4096):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array(values, dtype=np.uint64),
                           rng.integers(0, hi, n_random, dtype=np.uint64)]).astype(np.uint32).reshape(-1, 1)


def _split64(t):
    return [t & 0xFFFFFFFF, t >> 32]


def _lazy_case(acc0, mask, prods):
    assert len(prods) <= 8
    flat = [w for ab in prods for w in ab] + [0] * (16 - 2 * len(prods))
    return _split64(acc0) + [len(prods), mask] + flat


M1 = P - 1
CADENCE2 = 0b10101010  # lazy_fix after every second product: the loops of open.hip, jit.cpp emit_assert
CADENCE3 = 0b00100100


def lazy_cases():
    rng = np.random.default_rng(1305)
    top = P * R - 1  # the largest accumulator the invariant allows
    cases = [
        _lazy_case(0, 0, [(M1, M1)] * 4),                      # ef_mul: four products from 0, no fix in between
        _lazy_case(top, 0b10, [(M1, M1)] * 2),                 # two products on the largest accumulator, then fix
        _lazy_case(top, CADENCE2, [(M1, M1)] * 8),
        _lazy_case(0, CADENCE2, [(M1, M1)] * 8),
        _lazy_case(top, 0, []), _lazy_case(0, 0, []), _lazy_case(top, 1, [(0, 0)]),
        _lazy_case(top - (R - 1), 0b10, [(M1, M1)] * 2),       # high word p - 1, low word 0
        _lazy_case((P - 1) * R, 0b10, [(1, 1), (M1, 1)]),      # high word p - 1: the fix changes nothing
    ]
    for a in E[:: max(1, len(E) // 24)]:                       # edge factors against p - 1 on the largest accumulator
        cases.append(_lazy_case(top, CADENCE2, [(a, M1), (M1, a)] * 4))
    for _ in range(2048):
        acc0 = int(rng.integers(0, P, dtype=np.uint64)) * R + int(rng.integers(0, R, dtype=np.uint64))
        prods = [(int(a), int(b)) for a, b in rng.integers(P - (1 << 20), P, (8, 2), dtype=np.uint64)]
        cases.append(_lazy_case(acc0, CADENCE2, prods))
    for _ in range(2048):
        acc0 = int(rng.integers(0, P, dtype=np.uint64)) * R + int(rng.integers(0, R, dtype=np.uint64))
        prods = [(int(a), int(b)) for a, b in rng.integers(0, P, (8, 2), dtype=np.uint64)]
        cases.append(_lazy_case(acc0, CADENCE2, prods))
    return np.array(cases, dtype=np.uint64).astype(np.uint32)


def ef_elements():
    rng = np.random.default_rng(404)
    s = [(M1,) * 4, (0,) * 4, (R_MOD_P, 0, 0, 0), (1, 0, 0, 0), (P - R_MOD_P,) * 4]
    for k in range(4):
        for v in (1, M1, R_MOD_P):
            s.append(tuple(v if i == k else 0 for i in range(4)))
    win = [tuple(E[(i + j) % len(E)] for j in range(4)) for i in range(len(E))]
    rnd = [tuple(int(x) for x in r) for r in rng.integers(0, P, (1024, 4), dtype=np.uint64)]
    return s, win, rnd


def ef_pairs():
    s, win, rnd = ef_elements()
    pairs = [(a, b) for a in s for b in s]
    pairs += list(zip(win, reversed(win))) + list(zip(win, win))
    pairs += [(a, s[0]) for a in win[::4]] + [(s[0], a) for a in win[::4]]
    pairs += list(zip(rnd, reversed(rnd)))
    return np.array([a + b for a, b in pairs], dtype=np.uint64).astype(np.uint32)


def ef_singles():
    s, win, rnd = ef_elements()
    return np.array(s + win + rnd, dtype=np.uint64).astype(np.uint32)


def bitrev_cases():
    rng = np.random.default_rng(22)
    out = []
    for bits in list(range(28)) + [32]:
        m = (1 << bits) - 1
        xs = {0, 1, 2, 3, m, m >> 1, (m + 1) >> 1, 0x55555555 & m, 0xAAAAAAAA & m, 0x12345678 & m, 0xFFFFFFFF}
        xs |= {int(x) & m for x in rng.integers(0, R, 16, dtype=np.uint64)}
        out += [(x, bits) for x in sorted(xs)]
    return np.array(out, dtype=np.uint64).astype(np.uint32)


def _bitrev(x, bits):
    return int(format(x & ((1 << bits) - 1), f"0{bits}b")[::-1], 2) if bits else 0


def true_twiddles():
    """W[2^d + j] = w^bitrev(j, d) in Montgomery form, w of order 2^(d+1): the table layout of the NTT kernels
    for a 16-point transform (block j of stage d)."""
    w = [0] * 16
    for d in range(4):
        root = pow(G27, 1 << (27 - (d + 1)), P)
        for j in range(1 << d):
            w[(1 << d) + j] = pow(root, _bitrev(j, d), P) * R % P
    return w


def bfly_cases(top):
    """v[16] over [0, 2p) with the true twiddle table; without TOP also tables of edge values (TOP assumes
    W[2^d] = 1, which only a true table gives)."""
    rng = np.random.default_rng(1600 + top)
    tw = true_twiddles()
    vs = [[2 * P - 1] * 16, [0] * 16, [P] * 16, [P - 1] * 16, [2 * P - 2] * 16,
          [(2 * P - 1) * (q & 1) for q in range(16)], [(2 * P - 1) * ((q >> 3) & 1) for q in range(16)],
          [P * (q & 1) + (P - 1) for q in range(16)]]
    vs += [[LAZY[(i + 7 * q) % len(LAZY)] for q in range(16)] for i in range(len(LAZY))]
    vs += [[int(x) for x in r] for r in rng.integers(0, 2 * P, (1024, 16), dtype=np.uint64)]
    cases = [v + tw for v in vs]
    if not top:
        tables = [[M1] * 16, [0] * 16, [R_MOD_P] * 16, [P - R_MOD_P] * 16]
        tables += [[E[(i + 5 * q) % len(E)] for q in range(16)] for i in range(0, len(E), 8)]
        for t in tables:
            cases += [v + t for v in vs[:8] + vs[8::16]]
    return np.array(cases, dtype=np.uint64).astype(np.uint32)


def build_records(device):
    """{name: (n_in, n_out, operands (count, n_in) u32)} in file order."""
    rng = np.random.default_rng(7)
    exps = [0, 1, 2, 3, 5, P - 2, P - 1, P, (P - 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 63,
            0x123456789ABCDEF]
    t_values = [0, 1, P * R - 1, M1 * M1, R - 1, R, R + 1, P * R - R, (P - 1) * R, P, P - 1, R * R_MOD_P % (P * R)]
    t_values += [a * b for a in LAZY[::5] for b in E[::5]]
    t_values += [int(h) * R + int(l) for h, l in zip(rng.integers(0, P, 1 << 16, dtype=np.uint64),
                                                     rng.integers(0, R, 1 << 16, dtype=np.uint64))]
    s, win, rnd = ef_elements()
    pow_elems = s + win[::16] + rnd[:8]
    rec = {
        "consts": (1, 8, np.zeros((1, 1), dtype=np.uint32)),
        "add": (2, 1, _pairs(E, E, 1, P, P)),
        "sub": (2, 1, _pairs(E, E, 2, P, P)),
        "neg": (1, 1, _singles(E, 3, P)),
        "red2p": (1, 1, _singles(LAZY, 4, 2 * P)),
        "mont_reduce": (2, 1, np.array([_split64(t) for t in t_values], dtype=np.uint64).astype(np.uint32)),
        # a b < p 2^32: b < p, a any word
        "mont_mul": (2, 1, _pairs(LAZY + [1 << 31, R - 1], E, 6, R, P)),
        "to_mont": (1, 1, _singles(LAZY + [1 << 31, R - 1], 7, R)),
        "from_mont": (1, 1, _singles(LAZY + [1 << 31, R - 1], 8, R)),
        "mul": (2, 1, _pairs(E, E, 9, P, P)),
        "mont_inv": (1, 1, _singles(E, 10, P)),
        "inv_canon": (1, 1, _singles(E, 11, P)),
        "mont_mul_lazy": (2, 1, _pairs(LAZY, E, 12, 2 * P, P)),
        "lazy": (20, 3, lazy_cases()),
        # the control: the same largest operands at one lazy_fix per THREE products (see check_lazy_cadence3)
        "lazy_cadence3": (20, 3, np.array([_lazy_case(P * R - 1, CADENCE3, [(M1, M1)] * 6)],
                                          dtype=np.uint64).astype(np.uint32)),
        "ef_add": (8, 4, ef_pairs()),
        "ef_sub": (8, 4, ef_pairs()),
        "ef_neg": (4, 4, ef_singles()),
        "ef_mul": (8, 4, ef_pairs()),
        "ef_mul_base": (5, 4, np.array([a + (b,) for a in s + win[::8] + rnd[:64] for b in E[::3] + [M1]],
                                       dtype=np.uint64).astype(np.uint32)),
        "ef_inv_parts": (4, 5, ef_singles()),
        "ef_inv": (4, 4, ef_singles()),
        "ef_pow": (6, 4, np.array([list(a) + _split64(e) for a in pow_elems for e in exps[:-1]],
                                  dtype=np.uint64).astype(np.uint32)),
        "bitrev32": (2, 1, bitrev_cases()),
        "two_adic_generator": (1, 1, np.arange(28, dtype=np.uint32).reshape(-1, 1)),
        "pow_canon": (3, 1, np.array([[a] + _split64(e) for a in E[::7] + [M1] for e in exps],
                                     dtype=np.uint64).astype(np.uint32)),
        "mont_pow": (3, 1, np.array([[a] + _split64(e) for a in E[::7] + [M1] for e in exps],
                                    dtype=np.uint64).astype(np.uint32)),
    }
    if device:
        for name in DEVICE_ONLY:
            rec[name] = (32, 16, bfly_cases(name.endswith("_top")))
    return rec


# ------------------------------------------------------------------------------------------------ extreme matrices
EXTREME_KINDS = ["pm1", "zero", "alt_rows", "alt_cols"]


def extreme_mat(kind, h, w):
    """The matrices uniform data never produces, for the stage tests: every word p - 1, every word 0, and the
    two alternating by row and by column."""
    r, c = np.indices((h, w))
    pick = {"pm1": np.ones((h, w), bool), "zero": np.zeros((h, w), bool), "alt_rows": r % 2 == 1,
            "alt_cols": c % 2 == 1}[kind]
    return np.where(pick, P - 1, 0).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ probe I/O
def write_operands(path, records):
    words = [np.array([MAGIC, len(records)], dtype=np.uint32)]
    for name, (n_in, n_out, arr) in records.items():
        assert arr.dtype == np.uint32 and arr.ndim == 2 and arr.shape[1] == n_in, name
        words += [np.array([OPS[name], arr.shape[0], n_in, n_out], dtype=np.uint32), arr.reshape(-1)]
    np.concatenate(words).tofile(path)


def read_results(path, records):
    w = np.fromfile(path, dtype=np.uint32)
    assert w[0] == MAGIC and w[1] == len(records)
    pos, out = 2, {}
    for name, (n_in, n_out, arr) in records.items():
        assert (int(w[pos]), int(w[pos + 1]), int(w[pos + 2])) == (OPS[name], arr.shape[0], n_out), name
        out[name] = w[pos + 3: pos + 3 + arr.shape[0] * n_out].reshape(arr.shape[0], n_out)
        pos += 3 + arr.shape[0] * n_out
    assert pos == len(w)
    return out


def run_probe(tmp_dir, device):
    """One child process, one result file.  Returns (records, results)."""
    records = build_records(device)
    ops, res = os.path.join(tmp_dir, "operands.bin"), os.path.join(tmp_dir, "results.bin")
    write_operands(ops, records)
    cmd = [probe_path()] + ([] if device else ["--host"]) + [ops, res]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=PROBE_TIMEOUT_S)
    assert r.returncode == 0, f"field_probe exit {r.returncode}: {r.stderr.strip()}"
    return records, read_results(res, records)


# ------------------------------------------------------------------------------------------------ expectations
def _same(name, inp, got, want):
    """got (count, n_out) u32 against a list of expected rows (ints or tuples), exactly."""
    want = np.array(want, dtype=np.uint64).reshape(got.shape)
    bad = np.nonzero((got.astype(np.uint64) != want).any(axis=1))[0]
    assert len(bad) == 0, (f"{name}: {len(bad)} of {len(got)} operands wrong; first: in "
                           f"{[hex(int(x)) for x in inp[bad[0]]]} got {[hex(int(x)) for x in got[bad[0]]]} "
                           f"want {[hex(int(x)) for x in want[bad[0]]]}")


def _rows(inp):
    return [[int(x) for x in r] for r in inp]


def check_consts(inp, got):
    p, p_inv, p_neg_inv, r_mod_p, r2_mod_p, gen, g27, ef_w = (int(x) for x in got[0])
    assert p == P == 15 * (1 << 27) + 1
    assert p_inv == pow(P, -1, R) and p_neg_inv == (-pow(P, -1, R)) % R
    assert r_mod_p == R % P and r2_mod_p == R * R % P
    assert g27 == G27 and pow(g27, 1 << 27, P) == 1 and pow(g27, 1 << 26, P) != 1, "order must be exactly 2^27"
    # 31 generates F*: p - 1 = 2^27 * 3 * 5
    assert gen == 31 and all(pow(gen, (P - 1) // q, P) != 1 for q in (2, 3, 5))
    # x^4 - 11 is irreducible when 11 is not a square: with p = 1 mod 4 every -4 c^4 is a square, so the other
    # condition of the criterion for x^4 - a (a not of the form -4 c^4) follows
    assert ef_w == 11 and pow(11, (P - 1) // 2, P) == P - 1


def check_add(inp, got):
    _same("add", inp, got, [(a + b) % P for a, b in _rows(inp)])


def check_sub(inp, got):
    _same("sub", inp, got, [(a - b) % P for a, b in _rows(inp)])


def check_neg(inp, got):
    _same("neg", inp, got, [(-a) % P for a, in _rows(inp)])


def check_red2p(inp, got):
    _same("red2p", inp, got, [a % P for a, in _rows(inp)])


def check_mont_reduce(inp, got):
    _same("mont_reduce", inp, got, [(lo + (hi << 32)) * RINV % P for lo, hi in _rows(inp)])


def check_mont_mul(inp, got):
    _same("mont_mul", inp, got, [a * b * RINV % P for a, b in _rows(inp)])


def check_to_mont(inp, got):
    _same("to_mont", inp, got, [a * R % P for a, in _rows(inp)])


def check_from_mont(inp, got):
    _same("from_mont", inp, got, [a * RINV % P for a, in _rows(inp)])


def check_mul(inp, got):
    _same("mul", inp, got, [a * b % P for a, b in _rows(inp)])


def check_mont_inv(inp, got):
    # Montgomery in, Montgomery out: (a R^-1)^-1 R; the inverse of 0 is 0
    _same("mont_inv", inp, got, [pow(a, -1, P) * R * R % P if a else 0 for a, in _rows(inp)])


def check_inv_canon(inp, got):
    _same("inv_canon", inp, got, [pow(a, -1, P) if a else 0 for a, in _rows(inp)])


def check_mont_mul_lazy(inp, got):
    g = got[:, 0].astype(np.uint64)
    assert (g < 2 * P).all(), f"mont_mul_lazy: {int((g >= 2 * P).sum())} results outside [0, 2p)"
    _same("mont_mul_lazy (mod p)", inp, (g % np.uint64(P)).astype(np.uint32).reshape(-1, 1),
          [a * b * RINV % P for a, b in _rows(inp)])


def lazy_model(row, check_ranges=True):
    """(acc, finish) of one OP_LAZY item in unbounded integers; with check_ranges the preconditions of the
    bb.hpp comments are asserted on the way (acc < 2p 2^32 before a fix, acc < p 2^32 after it)."""
    acc, n, mask = row[0] + (row[1] << 32), row[2], row[3]
    for i in range(n):
        acc += row[4 + 2 * i] * row[5 + 2 * i]
        if (mask >> i) & 1:
            if check_ranges:
                assert acc < 2 * P * R, "operands break the precondition of lazy_fix"
            if (acc >> 32) >= P:
                acc -= P << 32
            if check_ranges:
                assert acc < P * R, "invariant acc < p 2^32 after lazy_fix"
    if check_ranges:
        assert acc < 2 * P * R
    return acc, acc * RINV % P


def check_lazy(inp, got):
    want = []
    for row in _rows(inp):
        acc, fin = lazy_model(row)
        want.append(_split64(acc) + [fin])
    _same("lazy_mac/lazy_fix/lazy_finish", inp, got, want)
    # the invariant itself, on what the code returned: after a final fix the accumulator is below p 2^32
    for row, g in zip(_rows(inp), got):
        if row[2] and (row[3] >> (row[2] - 1)) & 1:
            assert (int(g[1]) << 32) + int(g[0]) < P * R


def check_lazy_cadence3(inp, got):
    """Control for the operands: at one lazy_fix per three products the largest accumulator plus three products
    of (p-1)^2 passes 2p 2^32 (and 2^64), so the code's answer is NOT the sum any more.  If this ever holds,
    the `lazy` operands would no longer tell a cadence of three from the cadence of two."""
    row = _rows(inp)[0]
    acc, fin = lazy_model(row, check_ranges=False)
    first = row[0] + (row[1] << 32) + 3 * M1 * M1
    assert first >= 2 * P * R and first >= 1 << 64
    assert int(got[0][2]) != fin, "a cadence of three on the largest operands went unnoticed"


def ef_mul_int(a, b):
    r = [0] * 4
    for i in range(4):
        for j in range(4):
            r[(i + j) % 4] += a[i] * b[j] * (11 if i + j >= 4 else 1)
    return [x % P for x in r]


def ef_pow_int(a, e):
    r = [1, 0, 0, 0]
    while e:
        if e & 1:
            r = ef_mul_int(r, a)
        a = ef_mul_int(a, a)
        e >>= 1
    return r


def check_ef_add(inp, got):
    _same("ef_add", inp, got, [[(r[k] + r[4 + k]) % P for k in range(4)] for r in _rows(inp)])


def check_ef_sub(inp, got):
    _same("ef_sub", inp, got, [[(r[k] - r[4 + k]) % P for k in range(4)] for r in _rows(inp)])


def check_ef_neg(inp, got):
    _same("ef_neg", inp, got, [[(-x) % P for x in r] for r in _rows(inp)])


def check_ef_mul(inp, got):
    # Montgomery product: a b R^-1, whatever forms a and b are in
    _same("ef_mul", inp, got, [[x * RINV % P for x in ef_mul_int(r[:4], r[4:])] for r in _rows(inp)])


def check_ef_mul_base(inp, got):
    _same("ef_mul_base", inp, got, [[x * r[4] * RINV % P for x in r[:4]] for r in _rows(inp)])


def _canon(v):
    return [x * RINV % P for x in v]


def check_ef_inv_parts(inp, got):
    # Montgomery in and out: num nrm^-1 == a^-1, i.e. (num nrm^-1) a == 1 on the canonical values; a = 0
    # gives num = 0 and nrm = 0.  The inverse is unique, so this is equality with a^-1.
    bad = []
    for r, g in zip(_rows(inp), _rows(got)):
        a, num, nrm = _canon(r), _canon(g[:4]), g[4] * RINV % P
        if not any(a):
            ok = not any(num) and nrm == 0
        else:
            ok = nrm != 0 and max(g) < P and \
                ef_mul_int([x * pow(nrm, -1, P) % P for x in num], a) == [1, 0, 0, 0]
        if not ok:
            bad.append((r, g))
    assert not bad, f"ef_inv_parts: {len(bad)} wrong; first {bad[0]}"


def check_ef_inv(inp, got):
    bad = []
    for r, g in zip(_rows(inp), _rows(got)):
        a = _canon(r)
        ok = max(g) < P and (ef_mul_int(_canon(g), a) == [1, 0, 0, 0] if any(a) else not any(g))
        if not ok:
            bad.append((r, g))
    assert not bad, f"ef_inv: {len(bad)} wrong; first {bad[0]}"


def check_ef_pow(inp, got):
    _same("ef_pow", inp, got, [[x * R % P for x in ef_pow_int(_canon(r[:4]), r[4] + (r[5] << 32))]
                               for r in _rows(inp)])


def check_bitrev32(inp, got):
    _same("bitrev32", inp, got, [_bitrev(x, bits) for x, bits in _rows(inp)])


def check_two_adic_generator(inp, got):
    for (bits,), (g,) in zip(_rows(inp), _rows(got)):
        assert g == pow(G27, 1 << (27 - bits), P)
        assert pow(g, 1 << bits, P) == 1 and (bits == 0 or pow(g, 1 << (bits - 1), P) == P - 1)


def check_pow_canon(inp, got):
    _same("pow_canon", inp, got, [pow(a, lo + (hi << 32), P) for a, lo, hi in _rows(inp)])


def check_mont_pow(inp, got):
    _same("mont_pow", inp, got, [pow(a * RINV, lo + (hi << 32), P) * R % P for a, lo, hi in _rows(inp)])


def bfly_int(v, w, inverse):
    """The four radix-2 stages of one 16-point group, canonical integers; w[2^d + j] is the (canonical)
    twiddle of block j at stage d.  Forward: (a, b) -> (a + w b, a - w b); inverse: (a, b) -> (a + b, (a - b) w)."""
    v = list(v)
    for d in (range(3, -1, -1) if inverse else range(4)):
        half = 8 >> d
        for q in range(16):
            if q & half:
                continue
            tw = w[(1 << d) + (q >> (4 - d))]
            a, b = v[q], v[q + half]
            if inverse:
                v[q], v[q + half] = (a + b) % P, (a - b) * tw % P
            else:
                v[q], v[q + half] = (a + b * tw) % P, (a - b * tw) % P
    return v


def _check_bfly(name, inverse, inp, got):
    g = got.astype(np.uint64)
    assert (g < 2 * P).all(), f"{name}: {int((g >= 2 * P).any(axis=1).sum())} groups leave [0, 2p)"
    want = [bfly_int([x % P for x in r[:16]], _canon(r[16:]), inverse) for r in _rows(inp)]
    _same(name + " (mod p)", inp[:, :16], (g % np.uint64(P)).astype(np.uint32), want)


CHECKS = {name: globals()["check_" + name] for name in OPS if name not in DEVICE_ONLY}
CHECKS.update({"bfly_fwd": lambda i, g: _check_bfly("radix_butterflies<4, false, false>", False, i, g),
               "bfly_inv": lambda i, g: _check_bfly("radix_butterflies<4, true, false>", True, i, g),
               "bfly_fwd_top": lambda i, g: _check_bfly("radix_butterflies<4, false, true>", False, i, g),
               "bfly_inv_top": lambda i, g: _check_bfly("radix_butterflies<4, true, true>", True, i, g)})
HOST_NAMES = [n for n in OPS if n not in DEVICE_ONLY]
