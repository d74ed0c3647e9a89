"""The HOST build of the Plantard product of csrc/bb.hpp (P_INV64, plant_const, plant_mul) against plain Python
integers (tests/_plantard_cases.py), through the field probe's --host mode: no GPU.  The probe runs once per
module; all comparisons are exact."""
import pytest

import _plantard_cases as pc


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return pc.run_probe(str(tmp_path_factory.mktemp("plantard_host")), device=False)


def test_p_inv64(probe):
    records, _, results = probe
    pc.check_plant_consts(records["plant_consts"][2], results["plant_consts"])


def test_plant_const_matches_the_formula(probe):
    records, _, results = probe
    pc.check_plant_const(records["plant_const"][2], results["plant_const"])


def test_plant_mul_is_the_canonical_product_for_any_word(probe):
    records, _, results = probe
    inp = records["plant_mul"][2]
    # the operands the issue names are there: the ends of the 32-bit word, the lazy range's edges, w over E
    a = set(int(x) for x in inp[:, 0])
    assert {0, pc.P, pc.P + 1, 2 * pc.P - 1, 2 * pc.P, 1 << 31, pc.R - 2, pc.R - 1} <= a
    assert set(int(x) for x in inp[:, 1]) == set(pc.fc.E)
    pc.check_plant_mul(inp, results["plant_mul"])


def test_python_model_of_the_formula():
    """The expectation's own formula on the bound of the product: u = bits 32..63 of a W' mod 2^64,
    r = ((u + 1) p) >> 32, for the largest operands of both ranges."""
    for a in (0, 1, pc.P - 1, pc.P, 2 * pc.P - 1, pc.R - 1):
        for w in (0, 1, 2, pc.P - 1, (pc.P - 1) // 2):
            u = (a * pc.plant_const_int(w) % pc.R64) >> 32
            assert ((u + 1) * pc.P) >> 32 == a * w % pc.P
