"""The HOST build of every primitive of csrc/bb.hpp -- the constants, add/sub/neg, the Montgomery reductions and
inverses, the lazy 64-bit accumulators, EF4 and bitrev32 -- against plain Python integers, at the operands
where such code breaks (tests/_field_cases.py).  The field probe runs once with --host (no HIP call, no GPU);
every test reads its one result file.  All comparisons are exact.  tests/test_gpu_field.py is the same for the
device build."""
import pytest

import _field_cases as fc


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return fc.run_probe(str(tmp_path_factory.mktemp("field_host")), device=False)


@pytest.mark.parametrize("name", fc.HOST_NAMES)
def test_host_primitive(probe, name):
    records, results = probe
    fc.CHECKS[name](records[name][2], results[name])


def test_edge_set_is_what_the_module_says():
    e = set(fc.E)
    assert {0, 1, 2, fc.P - 2, fc.P - 1, (fc.P - 1) // 2, (fc.P + 1) // 2, fc.R % fc.P, fc.P - fc.R % fc.P} <= e
    assert all({1 << k, fc.P - (1 << k), (1 << k) - 1} <= e for k in range(31))
    # the Montgomery images: x R^-1 is an operand for every listed x, so x itself occurs as a Montgomery form
    assert all(((1 << k) * fc.RINV % fc.P in e) and ((fc.P - 1) * fc.RINV % fc.P in e) for k in range(31))
    assert max(e) < fc.P and len(fc.LAZY) == len(e) + 4


def test_probe_refuses_device_only_ops_and_bad_files(tmp_path):
    import subprocess

    records = {"bfly_fwd": (32, 16, fc.bfly_cases(False)[:1])}
    ops, res = str(tmp_path / "o.bin"), str(tmp_path / "r.bin")
    fc.write_operands(ops, records)
    r = subprocess.run([fc.probe_path(), "--host", ops, res], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "device build only" in r.stderr
    r = subprocess.run([fc.probe_path(), "--host", str(tmp_path / "missing.bin"), res], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "cannot read" in r.stderr
