"""The LDS bank model's byte form (tools/lds_quad_model.py): the ds_read_u8 of
the spread match window is conflict-free by layout for every group and any read
codes, a layout that put a group's lanes a byte apart would not be, and the
workgroup's 64-row table indexed by the absolute quality costs what the
per-wave 40-row table did (the swizzle nibble is q & 15 in both, and a row is
all 64 banks, so the row index does not pick the banks)."""
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


def test_byte_read_is_conflict_free_for_every_group():
    m = load_model()
    assert m.byte_read_cycles(np.random.default_rng(3), 500) == [1.0] * 16
    # the model does see conflicts in a byte read: lanes 256 bytes apart share a bank
    lanes = np.arange(64)[None, :]
    assert m.cycles(256 * lanes, m.B32_GROUPS, 4) == 64
    # lanes in one dword share a cycle (four lanes a dword: 16 dwords, 16 banks)
    assert m.cycles((lanes // 4) * 4, m.B32_GROUPS, 4) == 1


def test_window_addresses_cover_a_wave_once():
    m = load_model()
    code, lane, g = np.meshgrid(np.arange(5), np.arange(64), np.arange(16), indexing="ij")
    a = m.window_byte_addr(code, g, lane)
    assert len(np.unique(a)) == a.size and a.min() == 0 and a.max() == 5 * 64 * 16 - 1


def test_shared_table_costs_what_the_wave_table_did():
    m = load_model()
    q, _, pat4, r = m.draw(np.random.default_rng(7), 20000, 43, 73, 0.25)
    a = m.shared_table_addr(q, pat4)
    assert a.min() >= 0 and a.max() < 64 * 256 and not (a % 16).any()
    shared = float(m.cycles(a, m.B128_GROUPS, 16))
    wave = float(m.per_four_columns(r, pat4)[1])
    # another row-to-nibble assignment of the same draw: equal up to the seed-to-seed spread
    with open(os.path.join(ROOT, "profiles", "lds_quad128_model.jsonl")) as f:
        spread = json.loads(f.readlines()[1])["seed_to_seed"]
    assert abs(shared - wave) <= 4 * (spread["max"] - spread["min"]) + 0.05
    with open(os.path.join(ROOT, "profiles", "lds_byte_window_model.jsonl")) as f:
        rows = [json.loads(x) for x in f]
    assert rows[0]["lds_cycles_per_four_columns"] == round(shared, 2)
    assert rows[1]["lds_cycles_per_four_columns"] == 1.0
