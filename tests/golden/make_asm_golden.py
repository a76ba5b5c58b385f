"""Generate the fixture of the assembler's pin.

    make -C oracle oracle ref && python tests/golden/make_asm_golden.py

Writes tests/golden/asm_golden.npz: one array `cases` of UTF-8 JSON bytes holding
the inputs of tests/asm_pin_cases.py and what the REFERENCE does with them,
through its own headers compiled in place (oracle/ref_asm_driver.cpp ->
oracle/_ref/libref_asm.so). Data only: bytes as latin-1 text, scores as their 64
bits. The file is the same bytes on every run (fixed member date).

The generator refuses a fixture on which the reference threw, one that fails
the census of the families (asm_pin_cases.census), and one larger than twice
chain_golden.npz."""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import asm_pin_cases as P  # noqa: E402
import oracle  # noqa: E402

MAX_BYTES = 2 * os.path.getsize(os.path.join(HERE, "chain_golden.npz"))


def build():
    ref = oracle.AsmReference()
    rows = [(fam, name, reg, ref.assemble(reg["reads"], reg["ref"])) for fam, name, reg in P.all_cases()]
    names = [name for _, name, _, _ in rows]
    assert len(set(names)) == len(names), "duplicate case names"
    P.census({name: rec for _, name, _, rec in rows})
    return rows


def main():
    rows = build()
    P.write_fixture(rows, P.GOLDEN)
    size = os.path.getsize(P.GOLDEN)
    assert size <= MAX_BYTES, f"{size} bytes: more than twice chain_golden.npz ({MAX_BYTES})"
    back = P.load_fixture(P.GOLDEN)
    assert P.encode([(c["family"], c["name"], c["region"], c["record"]) for c in back]) == P.encode(rows)
    print(f"wrote {P.GOLDEN}: {len(rows)} cases, {size} bytes")


if __name__ == "__main__":
    main()
