"""The four single-table prove calls, ts_prove_batch_lookup, the four quotient_chunks and the four check_constraints
calls reproduce the fixture tests/golden/single_proofs_small.json word for word (tests/_single_cases.py; the host-only
half is tests/test_single_cpu.py).  The smallest shapes: nothing here depends on size."""
import numpy as np
import pytest

import tapstark_amd as ts
import _single_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lanes():
    from tapstark_amd.build import build

    build()
    ctxs = [ts.default_context()] + [ts.Context(0) for _ in range(3)]
    return {name: sc.Lane(ctx, sc.Statement(name)) for ctx, name in zip(ctxs, sc.CASE_NAMES)}


def _same(words, want):
    want = np.array(want, dtype=np.uint32)
    return len(words) == len(want) and bool((np.asarray(words) == want).all())


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_a_fresh_proof_equals_the_fixture(lanes, name):
    c = sc.load_golden()["cases"][name]
    ln = lanes[name]
    assert [int(x) for x in ln.st.tape] == c["tape"] and [int(x) for x in ln.st.pis] == c["public_values"]
    if ln.key is not None:
        assert [int(x) for x in ln.key.root] == c["key_root"]
    words = ln.prove()
    assert int(words[1]) == sc.VERSION[name]
    assert _same(words, c["proof"]), f"{name}: {int((words != np.array(c['proof'], dtype=np.uint32)).sum())} words differ"


def test_the_v1_fixture_is_the_oracles_proof(orc):
    st = sc.Statement("fib")
    want = orc.prove(orc.FriConfig(*sc.FRI), st.tape, st.trace, st.pis)
    assert _same(want, sc.load_golden()["cases"]["fib"]["proof"])


def test_the_batch_lanes_give_the_fixtures_v5_proofs(lanes):
    doc = sc.load_golden()
    got = sc.prove_batch([lanes[name] for name in sc.CASE_NAMES])
    for name, (words, exposed) in zip(sc.CASE_NAMES, got):
        c = doc["cases"][name]
        assert int(words[1]) == 5
        assert _same(words, c["batch_proof"]), f"{name}: the lane's proof differs from the fixture"
        assert [int(x) for x in exposed] == c["batch_exposed"]
    assert doc["cases"]["table"]["batch_proof"] == doc["cases"]["table"]["proof"]


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_quotient_chunks_and_check_constraints_equal_the_record(lanes, name):
    c = sc.load_golden()["cases"][name]
    digest, check, check_bad = lanes[name].stages()
    assert digest == c["chunks_sha256"]
    assert (check, check_bad) == (c["check"], c["check_bad"]) and check == -1 and check_bad >= 0
