"""Writes tests/golden/pre_aux_parent_programs.json: sha256 digests of the lowered program (ts_air_program) and of
the emitted source (ts_air_jit_source) of the pure-aux and pure-preprocessed splits of the seeded RandomAir family,
as the library lowered them BEFORE AIRs with both kinds of column existed.  Run it against a build of that
commit (its tree first on sys.path through TS_TREE); tests/test_air_pre_aux_cpu.py holds the current lowering to
these digests, so a tape with at most one of the two widths keeps its program word for word.

    TS_TREE=/path/to/that/checkout python tests/golden/make_pre_aux_parent_programs.py > \
        tests/golden/pre_aux_parent_programs.json
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("TS_TREE", os.path.dirname(os.path.dirname(HERE))))
import numpy as np

import tapstark_amd as ts
from tapstark_amd.airs import random_air_case
from _pre_aux_airs import split_tape_pre_aux, split_widths


def program_digest(prog) -> str:
    h = hashlib.sha256()
    h.update(np.uint32(prog["n_regs"]).tobytes())
    for k in ("code", "consts", "const_public"):
        h.update(np.ascontiguousarray(prog[k], dtype=np.uint32).tobytes())
    return h.hexdigest()


def digests(seed: int):
    air, _ = random_air_case(seed)
    w = air.width()
    if w < 3:
        return None
    p, a = split_widths(seed, w, 1)
    v1 = ts.air_tape(air, air.n_public)
    aux, pre = (ts.CompiledAir(None, split_tape_pre_aux(v1, 0, p + a)),
                ts.CompiledAir(None, split_tape_pre_aux(v1, p + a, 0)))
    return {"aux": program_digest(aux.program()), "pre": program_digest(pre.program()),
            "jit_aux": hashlib.sha256(aux.jit_source().encode()).hexdigest(),
            "jit_pre": hashlib.sha256(pre.jit_source().encode()).hexdigest()}


if __name__ == "__main__":
    out = {str(s): d for s in range(36) if (d := digests(s)) is not None}
    print(json.dumps(out, indent=0, sort_keys=True))
