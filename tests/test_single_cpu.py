"""The verify family of the single-table formats (TSPF v1, v3, v4, v5) and Proof.parse, without a GPU, on the
fixture tests/golden/single_proofs_small.json (tests/_single_cases.py writes it on a GPU).  What every ts_verify*
entry point answers -- status, verdict and the text of ts_last_error -- is the fixture's record."""
import numpy as np
import pytest

import tapstark_amd as ts
from tapstark_amd.stark import TSPF_MAGIC
import _single_cases as sc


@pytest.fixture(scope="module")
def doc():
    from tapstark_amd.build import build

    build()
    return sc.load_golden()


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_each_golden_is_accepted_by_its_own_entry_point(doc, name):
    c = doc["cases"][name]
    rc, verdict, text, exposed = sc.verify_call(sc.OWN_ENTRY[name], c["tape"], c["proof"], c["public_values"],
                                                c["key_root"])
    assert (rc, verdict, text) == (0, 0, "")
    assert [int(x) for x in exposed] == c["exposed"]
    assert doc["verify"][name][sc.OWN_ENTRY[name]] == [0, 0, ""]
    # the batch lanes' proof of the same statement is TSPF v5 whatever the AIR's widths
    rc, verdict, text, exposed = sc.verify_call("ts_verify_pre_aux", c["tape"], c["batch_proof"], c["public_values"],
                                                c["key_root"])
    assert (rc, verdict, text) == (0, 0, "") and [int(x) for x in exposed] == c["batch_exposed"] == c["exposed"]


@pytest.mark.parametrize("entry", sc.ENTRIES)
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_every_entry_point_answers_every_golden_as_recorded(doc, name, entry):
    c = doc["cases"][name]
    got = sc.verify_call(entry, c["tape"], c["proof"], c["public_values"], c["key_root"])[:3]
    assert list(got) == doc["verify"][name][entry]
    if entry != sc.OWN_ENTRY[name]:
        assert got[0] != 0, "another format's entry point took the proof"


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_refused_forms_give_the_recorded_triple(doc, name):
    c = doc["cases"][name]
    variants = sc.refusal_variants(name, c)
    assert [label for label, _, _ in variants] == list(doc["refusals"][name])
    for label, args, kw in variants:
        got = sc.verify_call(sc.OWN_ENTRY[name], *args, **kw)[:3]
        assert list(got) == doc["refusals"][name][label], label
        assert got[:2] != (0, 0), label


def test_the_verifier_is_clean_under_the_sanitizers(doc, tmp_path):
    """verifier.cpp, air.cpp and challenger.cpp built with AddressSanitizer and UBSan into the stand-alone program
    tap-stark_amd/probe/verify_probe.cpp (the rest comes from the product library), run on the four goldens and on
    their truncated and corrupted forms: every verdict is the recorded one and no sanitizer report ends the run."""
    import os
    import subprocess
    from tapstark_amd import build as b

    csrc = b.CSRC
    exe = str(tmp_path / "verify_probe")
    cmd = [b._clangxx(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(b._rocm(), "include"), "-I", csrc,
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(b.PKG, "probe", "verify_probe.cpp"),
           *(os.path.join(csrc, s) for s in ("verifier.cpp", "air.cpp", "challenger.cpp")), "-x", "none", b.build()]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out, n_records = [], 0
    for name, c in doc["cases"].items():
        records = [(c["proof"], 0)]
        for label, args, kw in sc.refusal_variants(name, c):
            if not kw and "root" not in label:  # a null root or exposed buffer is the C ABI's to refuse
                records.append(([int(x) for x in args[1]], doc["refusals"][name][label][1]))
        root = c["key_root"] or []
        for words, want in records:
            out += [c["version"], want, *doc["fri"], len(c["tape"]), len(c["public_values"]), 1 if root else 0,
                    len(words), *c["tape"], *c["public_values"], *root, *words]
            n_records += 1
    path = tmp_path / "cases.bin"
    np.array(out, dtype="<u4").tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert len(r.stdout.splitlines()) == n_records == 28


def _fri_tail_words(pf):
    out = [len(pf.commit_phase_commits), *pf.commit_phase_commits.reshape(-1), len(pf.query_proofs)]
    for q in pf.query_proofs:
        out.append(len(q.input_proof))
        for b in q.input_proof:
            out.append(len(b.opened_values))
            for v in b.opened_values:
                out += [len(v), *v]
            out += [len(b.opening_proof), *b.opening_proof.reshape(-1)]
        for vals, path in q.commit_phase_openings:
            out += [*vals.reshape(-1), len(path), *path.reshape(-1)]
    return out + [*pf.final_poly, pf.pow_witness]


@pytest.mark.parametrize("which", ["proof", "batch_proof"])
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_the_parsed_fields_are_the_words_in_wire_order(doc, name, which):
    words = np.array(doc["cases"][name][which], dtype=np.uint32)
    pf = ts.Proof.parse(words)
    v = pf.version
    assert v == (5 if which == "batch_proof" else sc.VERSION[name])
    width, qd = len(pf.trace_local), len(pf.quotient_chunks)
    out = [TSPF_MAGIC, v, pf.degree_bits, width, qd]
    if v == 3:
        out.append(pf.preprocessed_width)
    if v >= 4:
        out += [pf.aux_width, pf.n_challenges, len(pf.exposed)] + ([pf.preprocessed_width] if v == 5 else [])
    out += [*pf.trace_commit]
    if pf.aux_width:
        out += [*pf.aux_commit, *pf.exposed]
    else:
        assert pf.aux_commit is None and len(pf.exposed) == 0
    out += [*pf.quotient_commit]
    for m in (pf.preprocessed_local, pf.preprocessed_next, pf.aux_local, pf.aux_next, pf.trace_local, pf.trace_next,
              pf.quotient_chunks):
        out += [*m.reshape(-1)]
    out += _fri_tail_words(pf)
    assert np.array_equal(np.array(out, dtype=np.uint64), words)
    assert pf.preprocessed_local.shape == (pf.preprocessed_width, 4) and pf.aux_next.shape == (pf.aux_width, 4)
    assert pf.quotient_chunks.shape == (qd, 4, 4) and pf.trace_commit.shape == (8,)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_parse_refuses_a_truncated_and_an_overlong_proof(doc, name):
    words = np.array(doc["cases"][name]["proof"], dtype=np.uint32)
    for cut in (1, 5, len(words) // 2, len(words) - 1):
        with pytest.raises(ValueError):
            ts.Proof.parse(words[:cut])
    with pytest.raises(ValueError):
        ts.Proof.parse(np.append(words, np.uint32(0)))
    other = words.copy()
    other[1] = 6
    with pytest.raises(ValueError):
        ts.Proof.parse(other)
