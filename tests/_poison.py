"""Helper of tests/test_gpu_pool_poison.py: contexts whose device pool is filled with a test pattern
(TS_POOL_POISON, csrc/context.cpp) beside a clean one, and the comparison of one computation on all of them.

A block of the pool comes back as its last user left it, and the suite proves the same shapes over and over in
one context: a kernel or driver that skips a write, or reads past what was written, usually finds the right words
already there.  With the knob every block (the whole rounded block, first use and recycled) and every table holds
the word instead, so such a read changes the result.  Two words: 0x00000001 is canonical, unlike real data and
small should it ever be taken for an index or a count; 0xFFFFFFFF is above p and outside every lazy range.

Run as a program (`python tests/_poison.py NAME...`) it is the child process of the cases that depend on knobs
the library reads once per process: it runs the named cases of the test module on three contexts of its own and
prints a digest of each result."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tapstark_amd as ts  # noqa: E402

P = 0x78000001
KNOB = "TS_POOL_POISON"
WORDS = (None, "0x00000001", "0xFFFFFFFF")  # clean first: its first result is what every other one must equal
STAT_FILLS = 9  # ts_ctx_stat: blocks filled since the context was created


def rand_mat(seed, h, w):
    return np.random.default_rng(seed).integers(0, P, size=(h, w), dtype=np.uint32)


def make_contexts(count=None):
    """One context per word of WORDS -- or, with `count`, a list of that many per word (lanes, ranks) -- made
    with the knob set around the construction only."""
    out = []
    with pytest.MonkeyPatch.context() as mp:
        for word in WORDS:
            if word is None:
                mp.delenv(KNOB, raising=False)
            else:
                mp.setenv(KNOB, word)
            out.append(ts.Context(0) if count is None else [ts.Context(0) for _ in range(count)])
    return out


def fills(target) -> int:
    return sum(c.stat(STAT_FILLS) for c in (target if isinstance(target, list) else [target]))


def flat(x):
    """A result (arrays, bytes, integers, nested in lists, tuples and dicts) as a list of arrays."""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, (bytes, bytearray)):
        return [np.frombuffer(bytes(x), dtype=np.uint8)]
    if isinstance(x, (int, np.integer)):
        return [np.array([int(x)], dtype=np.int64)]
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for e in x for a in flat(e)]
    raise TypeError(f"no comparison for a {type(x).__name__}")


def digest(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def assert_same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} arrays for {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: array {i} has shape {g.shape}, not {w.shape}"
        bad = np.flatnonzero(np.asarray(g != w).reshape(-1))
        assert len(bad) == 0, (f"{what}: array {i} of shape {g.shape}: {len(bad)} words differ, first at flat index "
                               f"{int(bad[0])}: {int(g.reshape(-1)[bad[0]]):#x} for {int(w.reshape(-1)[bad[0]]):#x}")


def churn(ctx):
    """A call of another shape between the two runs of a case: the blocks the first run gave back are taken,
    written and given back again, so the second run works in recycled blocks that hold something else."""
    ctx = ctx[0] if isinstance(ctx, list) else ctx
    ts.Radix2Dft(ctx).coset_lde_batch(rand_mat(977, 1 << 9, 5), 1, 31).download()
    ts.Blake3Mmcs(ctx).commit([rand_mat(978, 1 << 6, 9)])


def same_everywhere(targets, fn, want=None, what=""):
    """fn(target) on the clean, the 0x00000001 and the 0xFFFFFFFF target in that order, twice each with a call of
    another shape in between (first-use and recycled blocks): every result equals, word for word, the clean
    target's first one and, where given, `want` (the oracle's); the poisoned targets filled blocks meanwhile and
    the clean one none.  Returns the result as a list of arrays."""
    ref = None
    for word, target in zip(WORDS, targets):
        before = fills(target)
        first = flat(fn(target))
        churn(target)
        second = flat(fn(target))
        filled = fills(target) - before
        name = "clean" if word is None else word
        if word is None:
            assert filled == 0, f"{what}: the clean context filled {filled} blocks"
            ref = first
        else:
            assert filled > 0, f"{what}: the {word} context filled no block"
        assert_same(first, ref, f"{what}: {name} context, first run, against the clean context")
        assert_same(second, ref, f"{what}: {name} context, second run, against the clean context")
    if want is not None:
        assert_same(ref, flat(want), f"{what}: against the oracle")
    return ref


def child_main(names):
    """The named cases of the test module, each through same_everywhere on contexts of this process."""
    import test_gpu_pool_poison as t

    from tapstark_amd.build import build

    build()
    targets = make_contexts()
    out = {}
    with pytest.MonkeyPatch.context() as env:
        for name in names:
            run = t.CASES[name][0]
            out[name] = digest(same_everywhere(targets, lambda c: run(c, env), what=name))
    print("POISON " + json.dumps(out), flush=True)


if __name__ == "__main__":
    child_main(sys.argv[1:])
