"""The executor's static plan (tf2_yolo_amd/plan.py) without a device: every graph and switch setting of
tests/golden/make_engine_plan.py is planned again and compared, row by row and field by field, with the digests in
tests/golden/engine_plan.json, which were taken from constructed Networks before the plan was split out of the executor. Needs only the built library."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_engine_plan as M   # noqa: E402
from tf2_yolo_amd import ops   # noqa: E402

with open(M.FIXTURE) as _f:
    GOLD = M.unpack(json.load(_f))   # {"graph|setting": {section: [row digests, column digests]}}


def _planned(monkeypatch, gname, sname):
    env = M.SETTINGS[sname]
    for k in [k for k in os.environ if k.startswith("YOLO_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(ops, "USE_PLANES", ops.CONV_MODE == "split" and env.get("YOLO_CONV_PLANES", "1") != "0")
    return M.plan_tables(gname)


def test_fixture_covers_every_graph_and_setting():
    assert sorted(GOLD) == sorted(f"{g}|{s}" for g in M.GRAPH_NAMES for s in M.SETTINGS)


def _chunks(text, n):
    return [text[i:i + n] for i in range(0, len(text), n)]


@pytest.mark.parametrize("sname", list(M.SETTINGS))
@pytest.mark.parametrize("gname", M.GRAPH_NAMES)
def test_plan_matches_the_recorded_plan(monkeypatch, gname, sname):
    """every row (a unit, a tensor, a total) and every field as recorded: a mismatch names the rows and the fields"""
    tab = _planned(monkeypatch, gname, sname)
    got, want, names = M.digests(tab), GOLD[f"{gname}|{sname}"], M.sections(tab)
    assert sorted(got) == sorted(want)
    bad = []
    for sec in want:
        if got[sec] == want[sec]:
            continue
        # (a row's digest covers its name: rows are looked up, not paired by position, so a row more or less shifts nothing)
        recorded, fields = set(_chunks(want[sec][0], 3)), M.FIELDS[sec.rstrip("0123456789")]
        rows = [name for (name, _), d in zip(names[sec], _chunks(got[sec][0], 3)) if d not in recorded]
        cols = [f for f, g, w in zip(fields, _chunks(got[sec][1], 6), _chunks(want[sec][1], 6)) if g != w]
        bad.append(f"{sec}: {len(names[sec])} rows planned, {len(want[sec][0]) // 3} recorded; rows not as recorded: {rows}; "
                   f"fields not as recorded: {cols}")
    assert not bad, f"{gname} under {sname}: " + "; ".join(bad)


def test_a_conv_output_that_is_a_network_output_keeps_its_fp32_copy(monkeypatch):
    """(the builders' outputs are head units: here a conv + BN unit whose only consumer reads planes is an output too)"""
    from tf2_yolo_amd import plan
    from tf2_yolo_amd.engine import GraphBuilder
    for k in [k for k in os.environ if k.startswith("YOLO_")]:
        monkeypatch.delenv(k)
    monkeypatch.setattr(ops, "USE_PLANES", ops.CONV_MODE == "split")

    def graph(as_output):
        b = GraphBuilder((16, 16, 32))
        x = b.conv(b.input, 32, 3, "c1")
        y = b.conv(x, 32, 3, "c2")
        b.head(b.conv(y, 32, 1, "c3"), 3, 11, 3, [(1, 1)] * 3, "out", level=0)   # 48 channels
        if as_output:
            b.outputs.append(x)
        plan.plan_graph(b.units, b.tensors, b.input, b.outputs, plan.Options.from_env())
        return b.units[0]
    assert graph(False).a_needed == (not ops.USE_PLANES)
    assert graph(True).a_needed is True


@pytest.mark.parametrize("sname", list(M.SETTINGS))
@pytest.mark.parametrize("gname", M.GRAPH_NAMES)
def test_filter_plane_regions_and_output_copies(monkeypatch, gname, sname):
    """by construction: the filter-plane regions of _wplanes are 256-byte aligned, disjoint and inside the total; the fp32
    form of every network output is written (a_needed of a conv unit, f32_needed of a pool or concat)"""
    tab = _planned(monkeypatch, gname, sname)   # (equal to the recorded plan: the test above)
    col = {f: i for i, f in enumerate(M.UNIT_FIELDS)}
    regions = []
    for key, row in tab.items():
        if not key.startswith("unit/"):
            continue
        for off, size in (("wp_off", "wp_bytes"), ("wTp_off", "wTp_bytes"), ("wTp_pad_off", "wTp_pad_bytes")):
            if row[col[size]] is not None:
                assert row[col[off]] % 256 == 0 and row[col[size]] > 0, (key, off)
                regions.append((row[col[off]], row[col[off]] + row[col[size]], key, off))
    regions.sort()
    for (_, end, key, what), (start, _, key2, what2) in zip(regions, regions[1:]):
        assert end <= start, f"{key} {what} overlaps {key2} {what2}"
    assert all(end <= tab["total/wplanes"][0] for _, end, _, _ in regions)
    assert bool(regions) == (tab["total/wplanes"][0] > 0)
    b = M._graphs()[gname]()
    for t in b.outputs:
        row = tab[f"unit/{t.producer.name}"]
        assert row[col["a_needed"]] in (None, 1) and row[col["f32_needed"]] in (None, 1), t.name
        if t.producer.kind == "conv":
            assert row[col["a_needed"]] == 1, t.name
