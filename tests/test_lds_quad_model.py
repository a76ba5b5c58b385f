"""The LDS bank model of the prior tables (tools/lds_quad_model.py): the
ds_read_b128 service groups partition the wave into four sets of 16 lanes, and
the two-read quad form still gives the committed 6.23 LDS cycles per read."""
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_model():
    spec = importlib.util.spec_from_file_location("lds_quad_model", os.path.join(ROOT, "tools", "lds_quad_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_b128_groups_partition_the_wave():
    m = load_model()
    assert len(m.B128_GROUPS) == 4
    assert all(len(g) == 16 and len(set(g)) == 16 for g in m.B128_GROUPS)
    assert sorted(l for g in m.B128_GROUPS for l in g) == list(range(64))
    assert [sorted(g) for g in m.B64_GROUPS] == [list(range(32)), list(range(32, 64))]


def test_conflict_free_and_broadcast_cycles():
    m = load_model()
    lanes = np.arange(64)[None, :]
    assert m.cycles(16 * (lanes % 16), m.B128_GROUPS, 16) == 4      # 16 slots of one row: one cycle a group
    assert m.cycles(np.zeros((1, 64), np.int64), m.B128_GROUPS, 16) == 4   # one address: broadcast
    assert m.cycles(256 * lanes, m.B128_GROUPS, 16) == 64           # one slot of 64 rows: 16-way in every group
    assert m.cycles(8 * (lanes % 32)) == 2


def test_two_read_form_gives_the_committed_figure():
    m = load_model()
    q, _, pat4, r = m.draw(np.random.default_rng(7), 20000, 43, 73, 0.25)
    two = m.cycles(128 * r + 8 * (pat4 ^ ((r >> 1) & 15)))
    assert round(float(two), 2) == 6.23
    with open(os.path.join(ROOT, "profiles", "lds_quad_model.jsonl")) as f:
        rows = [json.loads(x) for x in f]
    assert rows[2]["lds_cycles_per_read"] == 6.23
    with open(os.path.join(ROOT, "profiles", "lds_quad128_model.jsonl")) as f:
        rows128 = [json.loads(x) for x in f]
    assert rows128[0]["lds_cycles_per_read"] == 6.23
    assert round(float(m.per_four_columns(r, pat4)[1]), 2) == rows128[1]["lds_cycles_per_four_columns"]
