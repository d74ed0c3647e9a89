"""The DEVICE build of every primitive of csrc/bb.hpp and of the register butterflies of csrc/ntt_rounds.hpp
against plain Python integers (tests/_field_cases.py): the operands and expectations of tests/test_field_cpu.py,
plus radix_butterflies<4, INV, TOP> over the lazy range [0, 2p).  The field probe runs ONCE per module, as a
child process with its own time limit and one kernel launch per operation; every test reads its one result
file, and if the child fails the fixture fails and nothing starts it again.  All comparisons are exact."""
import pytest

import _field_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return fc.run_probe(str(tmp_path_factory.mktemp("field_device")), device=True)


@pytest.mark.parametrize("name", fc.HOST_NAMES + list(fc.DEVICE_ONLY))
def test_device_primitive(probe, name):
    records, results = probe
    fc.CHECKS[name](records[name][2], results[name])
