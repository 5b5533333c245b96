"""GPU-free guards of the "past the grid cap" tests (tests/past_cap_cases.py):

  * the two caps are read from the sources (stream_grid in csrc/common.hpp, `blocks > N` in the two launchers of
    csrc/loss.hip; the danchor cap from csrc/elementwise.hip) and every case of the table is checked against them -- a later
    change of a cap must not turn those tests back into one-pass tests unnoticed;
  * for every loss case, the discrete decisions (responsible anchor, ignore / truth masks) that OL.cal_iou gives in float32
    and in float64 on the CPU are the same in EVERY cell: a disagreement of the device with the float64 oracle about a
    decision is then a fault of the kernel, not a threshold coin-flip of the inputs."""
import os
import re

import pytest
import torch

import past_cap_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tf2_yolo_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _stream_cap():
    m = re.search(r"inline int stream_grid\(long long work_items, int block\)\s*\{(.*?)\n\}", _read("common.hpp"), re.S)
    assert m, "stream_grid() not found in csrc/common.hpp: revisit GLUE_CASES / STREAM_CAP of tests/past_cap_cases.py"
    caps = re.findall(r"if \(g > (\d+)\) g = (\d+);", m.group(1))
    assert len(caps) == 1 and caps[0][0] == caps[0][1], \
        "the cap of stream_grid() changed its form: revisit GLUE_CASES / STREAM_CAP of tests/past_cap_cases.py"
    return int(caps[0][0])


def _loss_caps():
    src = _read("loss.hip")
    caps = re.findall(r"if \(blocks > (\d+)\) blocks = (\d+);", src)
    assert len(caps) == 2 and all(a == b for a, b in caps), \
        "`blocks > N` of yolo_loss_fwd_bwd / yolo_metrics not found: revisit LOSS_CASES / LOSS_CAP of tests/past_cap_cases.py"
    per = re.findall(r"long long blocks = \(lp\.cells \+ (\d+)\) / (\d+);", src)
    assert len(per) == 2 and all(int(a) + 1 == int(b) for a, b in per), \
        "cells per workgroup of the loss launchers not found: revisit LOSS_CASES / LOSS_CAP of tests/past_cap_cases.py"
    return [int(c[0]) * int(p[1]) for c, p in zip(caps, per)]


def _danchor_cap():
    m = re.search(r"long long gx = \(P \+ 255\) / 256;\s*if \(gx > (\d+)\) gx = (\d+);", _read("elementwise.hip"))
    assert m and m.group(1) == m.group(2), \
        "the cap of head_danchor_kernel not found: revisit head_v4_danchors / DANCHOR_CAP of tests/past_cap_cases.py"
    return int(m.group(1)) * 256


def test_caps_in_the_sources_are_the_caps_of_the_table():
    assert _stream_cap() * PC.STREAM_BLOCK == PC.STREAM_CAP == 524288
    assert _loss_caps() == [PC.LOSS_CAP, PC.LOSS_CAP] and PC.LOSS_CAP == 8192
    assert _danchor_cap() == PC.DANCHOR_CAP
    # every launcher of a table case sizes its grid with stream_grid(..., 256)
    for name in ("elementwise.hip", "bn_act.hip", "labels.hip", "iou.hip"):
        blocks = set(re.findall(r"stream_grid\([^;]*?, (\d+)\)", _read(name)))
        assert blocks <= {"256"}, (name, blocks)


@pytest.mark.parametrize("case", PC.GLUE_CASES, ids=lambda c: c.name)
def test_glue_case_runs_three_passes_the_last_one_partial(case):
    cap = {PC.STREAM_CAP: _stream_cap() * PC.STREAM_BLOCK, PC.DANCHOR_CAP: _danchor_cap()}[case.cap]
    assert 2 * cap < case.items <= 3 * cap, (case.name, case.items, cap)
    assert case.items % cap != 0


@pytest.mark.parametrize("case", PC.LOSS_CASES, ids=lambda c: c.name)
def test_loss_case_lies_in_its_band(case):
    cap = min(_loss_caps())
    cells = PC.loss_cells(case)
    if case.band == 3:
        assert 2 * cap < cells <= 3 * cap and 2 * max(_loss_caps()) < cells
    else:
        assert case.band == 2 and cap < cells < 2 * cap
    assert cells % cap != 0
    # which loader the launcher picks: a whole cell ahead needs at most 256 prediction channels
    assert (PC.loss_pred_channels(case) > 256) == (case.name == "v3-c91")


def test_table_names_every_band_and_every_version():
    assert {c.version for c in PC.LOSS_CASES} == {1, 2, 3, 4}
    assert {c.band for c in PC.LOSS_CASES} == {2, 3}
    assert any(c.g[0] != c.g[1] for c in PC.LOSS_CASES)
    for n in PC.LOSS_CHUNK_AHEAD + PC.LOSS_NO_GRAD + PC.METRICS_CASES + [PC.LOSS_GRAD_SCALE]:
        assert n in PC.LOSS_BY_NAME
    assert {PC.LOSS_BY_NAME[n].version for n in PC.METRICS_CASES} == {1, 2, 3, 4}


@pytest.mark.parametrize("case", PC.LOSS_CASES, ids=lambda c: c.name)
def test_loss_case_decisions_do_not_depend_on_the_precision(case):
    i32, _ = PC.loss_case_ious(case, torch.float32)
    i64, obj = PC.loss_case_ious(case, torch.float64)
    truth = case.kw.get("truth_thresh", 1.0)
    d32, d64 = PC.decisions_of(i32, 0.6, truth), PC.decisions_of(i64, 0.6, truth)
    differ = int((d32 != d64).any(1).sum())
    fired = int(((i64 >= 0.6).any(1) & (obj > 0)).sum())
    print(f"PAST_CAP_DECISIONS {case.name}: {differ} of {d64.shape[0]} cells differ between float32 and float64; "
          f"{fired} object cells have an IoU above 0.6")
    assert differ == 0
    if case.version != 1:
        assert fired > 500            # the masks are exercised
