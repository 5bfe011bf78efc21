"""Every operation of every engine instantiation on the device against the oracle's C restatement, cell by cell (tests/engine_cells.py:
34 instantiations x 10 rows, the table tests/test_engine_cells_table.py checks against the sources).

One test per instantiation.  For every row it asks pmx_ctx_engine_info for the shape it is about to launch and requires the intended engine
- `HybridEngine<t,5,` / `HybridEngine<t,0,` (with ` x passes` on the absorb / squeeze rows and only there), `QuadEngine<a>`, `LdsEngine<a>` -
and the Montgomery step that follows from the config's modulus; then the call runs through its public entry point and every output, end
state and mode word must equal the C port limb for limb: nodes and roots of the tree rows, `found` and `nonce` of the grind row (whose
range provably holds two accepted nonces, the smallest beyond the first wave).  test_no_cell_is_empty closes the table: every cell was
asked and answered by the intended engine, and a cell whose instantiation ran here was compared."""
import time

import pytest

import engine_cells as E

pytestmark = pytest.mark.gpu

# (instantiation id, row) -> (engine string, p1 of the config's modulus, compared) as the tests below met them
ANSWERED = {}


def ask(c):
    """the library's answer for the cell's launch, recorded; asserts it is the intended engine"""
    name = E.engine_answer(c)
    p1 = E.p1_of(E.product_config(c.inst, c.rate, c.capacity).field.modulus)
    key = (E.inst_id(c.inst), c.row)
    ANSWERED[key] = (name, p1, ANSWERED.get(key, (None, None, False))[2])
    assert E.engine_matches(c.inst, c.row, name), (key, name, E.intended_engine(c.inst, c.row))
    assert p1 == c.inst.p1, (key, "the config's modulus takes the other Montgomery step")
    return name


@pytest.mark.parametrize("ident", [E.inst_id(i) for i in E.INSTANTIATIONS])
def test_every_row_equals_the_c_port(ident):
    inst = E.BY_ID[ident]
    started = time.perf_counter()
    names, differing = set(), []
    for row in E.ROWS:
        c = E.cell(inst, row)
        if c is None:
            assert (ident, row) in E.UNREACHABLE
            continue
        if row == "grind":
            E.assert_grind_searches(c)
        want = E.expected(c)
        names.add(ask(c).decode())
        got = E.run(c)
        differing += [(row, output) for output in E.differences(got, want)]      # (the rows behind a wrong one are still compared)
        ANSWERED[(ident, row)] = ANSWERED[(ident, row)][:2] + (True,)
    print("%-24s %6.2f s  %s" % (ident, time.perf_counter() - started, " | ".join(sorted(names))))
    assert differing == [], (ident, "outputs that differ from the C port")


def test_no_cell_is_empty():
    ran = {ident for ident, _ in ANSWERED}
    wrong, not_compared = [], []
    for c in E.cells():
        key = (E.inst_id(c.inst), c.row)
        if key not in ANSWERED:                 # (this test selected alone, or another worker ran the cell: ask the shape again)
            ANSWERED[key] = (E.engine_answer(c), E.p1_of(E.product_config(c.inst, c.rate, c.capacity).field.modulus), False)
        name, p1, compared = ANSWERED[key]
        if not E.engine_matches(c.inst, c.row, name) or p1 != c.inst.p1:
            wrong.append((key, name, p1))
        if key[0] in ran and not compared:
            not_compared.append(key)
    assert wrong == [], "cells the library would launch on another engine or Montgomery step"
    assert not_compared == [], "cells of an instantiation that ran here but were not compared with the C port"
    assert set(ANSWERED) == {(E.inst_id(c.inst), c.row) for c in E.cells()}
    assert len(ANSWERED) + len(E.UNREACHABLE) == len(E.INSTANTIATIONS) * len(E.ROWS)
