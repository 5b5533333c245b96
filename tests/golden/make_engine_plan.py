"""Generator of tests/golden/engine_plan.json: the static plan of the executor (tf2_yolo_amd/plan.py) for six small
graphs under seven switch settings, as plain tables keyed by unit and tensor names. Runs on the CPU: it needs the built
library for the host-side queries (planes_bytes, bnred_slots_cap) and no device.

    python tests/golden/make_engine_plan.py          # rewrites engine_plan.json next to this file

The committed file was first taken from constructed Networks of the commit before plan.py existed (on the GPU, once) and
is byte-identical to what this script writes: tests/test_plan_cpu.py keeps it so.

The file holds digests, not the tables (260 KB of them): {"<graph>|<setting>": {"<section>": [rows, columns]}}. `rows` is
3 hex digits per row of the section, in the order of `tables` (name and values: they say WHICH unit or tensor differs),
`columns` 6 hex digits per field over all rows (they say WHICH field, and are what makes a missed difference unlikely:
2^-24 per field). Sections of a non-default setting that equal the same graph's "default" are left out."""
import contextlib
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FIXTURE = os.path.join(HERE, "engine_plan.json")

V2_ANCHORS = [[0.57273, 0.677385], [1.87446, 2.06253], [3.33843, 5.47434], [7.88282, 3.52778], [9.77052, 9.16828]]


def _graphs():
    from tf2_yolo_amd import graphs as G
    return {
        "v3": lambda: G.build_yolov3((64, 64, 3), 3),
        "v3tiny": lambda: G.build_yolov3((64, 64, 3), 3, anchors=G.V3_DEFAULT_ANCHORS[:6], backbone="tiny_darknet"),
        "v4": lambda: G.build_yolov4((64, 64, 3), 3),
        "v2": lambda: G.build_yolov2((64, 64, 3), 3, V2_ANCHORS),
        "v1_5": lambda: G.build_yolov1_5((128, 128, 3), 1, 2),
        "v3_80": lambda: G.build_yolov3((64, 96, 3), 80),
    }


GRAPH_NAMES = ["v3", "v3tiny", "v4", "v2", "v1_5", "v3_80"]

SETTINGS = {
    "default": {},
    "conv_planes0": {"YOLO_CONV_PLANES": "0"},
    "fused_reduce1": {"YOLO_BN_FUSED_REDUCE": "1"},
    "fused_reduce_ws": {"YOLO_BN_FUSED_REDUCE": "ws"},
    "fused_reduce_t": {"YOLO_BN_FUSED_REDUCE": "t"},
    "dyp_per_layer0": {"YOLO_DYP_PER_LAYER": "0"},
    "all_off": {"YOLO_RES_PLANES": "0", "YOLO_HEAD_PAD": "0", "YOLO_POOL_FUSE": "0", "YOLO_CONCAT_PLANES": "0",
                "YOLO_DGRAD_CLASSES": "0"},
}

BATCHES = (1, 2)

UNIT_FIELDS = ["planes_fwd", "planes_dgrad", "planes_wgrad", "cpad", "wp_off", "wp_bytes", "wTp_off", "wTp_bytes",
               "wTp_pad_off", "wTp_pad_bytes", "a_needed", "f32_needed", "pool_fuse", "aux_off", "pred_off", "wT_off",
               "bn_f32_off", "bn_f64_off", "bn_red_off", "bnred_for", "bnred_class"]


def _plain(v):
    if v is None or isinstance(v, str):
        return v
    if hasattr(v, "name"):      # a unit
        return v.name
    return int(v)


def unit_row(u):
    """UNIT_FIELDS of one unit as the plan left them on it (None: not set for this unit). Sizes of regions a unit does
    not have are not part of the plan: they read None whatever is stored."""
    row = {f: _plain(getattr(u, f, None)) for f in UNIT_FIELDS}
    if not row["planes_fwd"]:
        row["wp_bytes"] = None
    if not row["planes_dgrad"]:
        row["wTp_bytes"] = None
    if not row["cpad"]:
        row["wTp_pad_off"] = row["wTp_pad_bytes"] = None
    return [row[f] for f in UNIT_FIELDS]


def desc_row(d):
    return None if d is None else [int(getattr(d, f)) for f, _ in d._fields_]


def tables(units, tensors, graph, batches):
    """{"section/name": row} of one graph under one setting.
      unit/<unit>          UNIT_FIELDS
      tensor/<tid>:<name>  [needs_grad, n_consumers, [consumer units], bound_alias tensor or None, read-through upsample or None]
      total/<what>         [value]: wplanes, aux, tbound_off, wT, bn_f32, bn_f64, bn_stats, pred
      desc<N>/<unit>       [desc, desc_pad, [pad_t, pad_l] of a pool]
      bytes<N>/<unit>      [planes of its output (None: none kept), its own dy planes, BnReduce slot capacity (None: none)]
      bytes<N>/shared_dyp  [bytes of one buffer of the shared pair]
    graph: needs_grad, n_consumers, consumers, bound_alias, up_producer keyed by tid, and totals;
    batches[N]: desc, desc_pad, pool_pad, dyp_own, bnred_cap keyed by unit name, xplanes by tid, dyp_shared."""
    names = [u.name for u in units]
    assert len(set(names)) == len(names), "unit names must be unique"
    tname = {t.tid: f"{t.tid}:{t.name}" for t in tensors}
    out = {}
    for u in units:
        out[f"unit/{u.name}"] = unit_row(u)
    for t in tensors:
        alias = graph["bound_alias"].get(t.tid)
        up = graph["up_producer"].get(t.tid)
        out[f"tensor/{tname[t.tid]}"] = [_plain(graph["needs_grad"][t.tid]), int(graph["n_consumers"].get(t.tid, 0)),
                                         [c.name for c in graph["consumers"].get(t.tid, [])],
                                         None if alias is None else tname[alias], None if up is None else up.name]
    for k, v in graph["totals"].items():
        out[f"total/{k}"] = [int(v)]
    for N, b in batches.items():
        for u in units:
            pads = b["pool_pad"].get(u.name)
            row = [desc_row(b["desc"].get(u.name)), desc_row(b["desc_pad"].get(u.name)), None if pads is None else list(pads)]
            if any(r is not None for r in row):
                out[f"desc{N}/{u.name}"] = row
            row = [b["xplanes"].get(u.out.tid), b["dyp_own"].get(u.name), b["bnred_cap"].get(u.name)]
            if any(r is not None for r in row):
                out[f"bytes{N}/{u.name}"] = [None if r is None else int(r) for r in row]
        out[f"bytes{N}/shared_dyp"] = [int(b["dyp_shared"])]
    return out


@contextlib.contextmanager
def setting_env(env):
    """the YOLO_* variables of one setting (everything else of YOLO_* unset) and ops.USE_PLANES, restored afterwards"""
    from tf2_yolo_amd import ops
    saved = {k: v for k, v in os.environ.items() if k.startswith("YOLO_")}
    saved_planes = ops.USE_PLANES
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    ops.USE_PLANES = ops.CONV_MODE == "split" and env.get("YOLO_CONV_PLANES", "1") != "0"
    try:
        yield
    finally:
        ops.USE_PLANES = saved_planes
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def plan_tables(graph_name):
    """the tables of one graph under the switches of the environment as it is now (plan.py, no device)"""
    from tf2_yolo_amd import plan
    b = _graphs()[graph_name]()
    opts = plan.Options.from_env()
    g = plan.plan_graph(b.units, b.tensors, b.input, b.outputs, opts)
    graph = {"needs_grad": g.needs_grad, "n_consumers": g.n_consumers, "consumers": g.consumers,
             "bound_alias": g.bound_alias, "up_producer": g.up_producer,
             "totals": {"wplanes": g.wplanes_total, "aux": g.aux_total, "tbound_off": g.tbound_off, "wT": g.wT_total,
                        "bn_f32": g.bn_f32_total, "bn_f64": g.bn_f64_total, "bn_stats": g.bn_stats_total,
                        "pred": g.pred_total}}
    batches = {}
    for N in BATCHES:
        p = plan.plan_batch(b.units, N, opts)
        batches[N] = {"desc": p.desc, "desc_pad": p.desc_pad, "pool_pad": p.pool_pad, "dyp_own": p.dyp_own_bytes,
                      "bnred_cap": p.bnred_cap, "xplanes": p.xplanes_bytes, "dyp_shared": p.dyp_shared_bytes}
    return tables(b.units, b.tensors, graph, batches)


# the fields of a row, per section (desc<N> / bytes<N>: see `tables`)
FIELDS = {"unit": UNIT_FIELDS, "tensor": ["needs_grad", "n_consumers", "consumers", "bound_alias", "up_producer"],
          "total": ["value"], "desc": ["desc", "desc_pad", "pool_pad"], "bytes": ["planes / shared", "dyp_own", "bnred_cap"]}


def _digest(obj, n):
    return hashlib.sha1(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()[:n]


def sections(tab):
    """{"section/name": row} -> {section: [(name, row)]} in the order of `tables`"""
    out = {}
    for key, row in tab.items():
        sec, name = key.split("/", 1)
        out.setdefault(sec, []).append((name, row))
    return out


def digests(tab):
    """{section: [rows, columns]} of one config (module docstring)"""
    out = {}
    for sec, rows in sections(tab).items():
        width = max(len(r) for _, r in rows)
        cols = [[r[i] if i < len(r) else None for _, r in rows] for i in range(width)]
        out[sec] = ["".join(_digest([name, r], 3) for name, r in rows), "".join(_digest(c, 6) for c in cols)]
    return out


def pack(full):
    """{"graph|setting": tables} -> the stored form"""
    out = {}
    for key, tab in full.items():
        graph, setting = key.split("|")
        d = digests(tab)
        if setting != "default":
            base = digests(full[f"{graph}|default"])
            d = {sec: v for sec, v in d.items() if base.get(sec) != v}
        out[key] = d
    return out


def unpack(stored):
    return {key: dict(stored[key.split("|")[0] + "|default"], **d) for key, d in stored.items()}


def write_fixture(full, path):
    with open(path, "w") as f:
        rows = [f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'), sort_keys=True)}" for k, v in sorted(pack(full).items())]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")   # one line per config


def main():
    full = {}
    for gname in GRAPH_NAMES:
        for sname, env in SETTINGS.items():
            with setting_env(env):
                full[f"{gname}|{sname}"] = plan_tables(gname)
    write_fixture(full, FIXTURE)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, {len(full)} configs")


if __name__ == "__main__":
    main()
