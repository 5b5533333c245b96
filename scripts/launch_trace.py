"""What the executor launches, as text: one line per entry of the launch tape (tape.py) for a few fixed scenarios, so that two
commits can be compared with `diff -r` -- a refactor of engine.py must leave every line as it was.

    python scripts/launch_trace.py OUTDIR            # every graph and setting, one fresh child process each
    python scripts/launch_trace.py OUTDIR child GRAPH SETTING BATCH

It uses only what any commit has: tape.ACTIVE (every enqueueing library call is remembered with its arguments, and ops._p
keeps every tensor alive, so no address is reused while a scenario records), the Network's flat buffers and the builders.

A line is the call's name and its arguments: scalars as they are; a structure passed by reference field by field (a
scalar passed by reference, which the call fills in, as `out`); an array element by element; a pointer into one of the
Network's flat buffers as <buffer>+<byte offset>; any other pointer or stream as #<rank of its first appearance in the
process>; a Python entry (stream / event operation, torch copy, hook) as `py`.

Scenarios at batch 2 (seeded input and output gradients): (1) forward(training=True) + backward, (2) the same again with
the filter planes valid, (3) mark_params_changed() and once more, (4) forward(training=False) twice. At batch 1, in a
second process: forward(training=False) twice (small tiles, head units, read-through upsampling)."""
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2_ANCHORS = [[0.57273, 0.677385], [1.87446, 2.06253], [3.33843, 5.47434], [7.88282, 3.52778], [9.77052, 9.16828]]
GRAPHS = ["v3", "v3tiny", "v4", "v2", "v1_5"]
SETTINGS = {
    "default": {},
    "conv_planes0": {"YOLO_CONV_PLANES": "0"},
    "fused_reduce1": {"YOLO_BN_FUSED_REDUCE": "1"},
    "dyp_per_layer0": {"YOLO_DYP_PER_LAYER": "0"},
    "infer_fuse0": {"YOLO_INFER_FUSE": "0"},
    "bwd_overlap0": {"YOLO_BWD_OVERLAP": "0"},
}
FLAT = ["params.data", "state.data", "grads", "_wT", "_wplanes", "_aux", "_bn_f32", "_bn_f64", "_pred", "_twords",
        "anchors_flat", "anchor_grads"]
CHILD_TIMEOUT = 240


def build(name):
    from tf2_yolo_amd import graphs as G
    if name == "v3":
        return G.build_yolov3((64, 64, 3), 3)
    if name == "v3tiny":
        return G.build_yolov3((64, 64, 3), 3, anchors=G.V3_DEFAULT_ANCHORS[:6], backbone="tiny_darknet")
    if name == "v4":
        return G.build_yolov4((64, 64, 3), 3)
    if name == "v2":
        return G.build_yolov2((64, 64, 3), 3, V2_ANCHORS)
    if name == "v1_5":
        return G.build_yolov1_5((128, 128, 3), 1, 2)
    raise ValueError(name)


class Renderer:
    def __init__(self, net):
        self.net = net
        self.ranks = {}

    def _buffers(self):
        out = []
        for name in FLAT:
            t = self.net
            for part in name.split("."):
                t = getattr(t, part, None)
            if t is not None:
                out.append((name, t.data_ptr(), t.numel() * t.element_size()))
        return out

    def _ptr(self, v, bufs):
        if not v:
            return "null"
        for name, base, n in bufs:
            if base <= v < base + n:
                return f"{name}+{v - base}"
        return f"#{self.ranks.setdefault(v, len(self.ranks))}"

    def _arg(self, a, bufs):
        if isinstance(a, ctypes.c_void_p):
            return self._ptr(a.value, bufs)
        if hasattr(a, "_obj"):     # byref(structure), or byref(scalar) that the call fills in
            s = a._obj
            if not isinstance(s, ctypes.Structure):
                return "out"
            return "{" + ",".join(f"{f}={getattr(s, f)}" for f, _ in s._fields_) + "}"
        if isinstance(a, ctypes.Array):   # (its own address is the host's: only what it holds is written)
            pointers = issubclass(a._type_, ctypes.c_void_p)
            return "[" + ",".join(self._ptr(v, bufs) if pointers else repr(v) for v in a) + "]"
        if isinstance(a, ctypes._SimpleCData):
            return repr(a.value)
        return repr(a)

    def lines(self, t):
        bufs = self._buffers()
        for f, a, name in t.entries:
            yield "py" if f is None else name + " " + " ".join(self._arg(x, bufs) for x in a)


def child(outdir, gname, sname, batch):
    import torch
    from tf2_yolo_amd import tape
    from tf2_yolo_amd.engine import Network
    torch.cuda.set_device(0)
    net = Network(build(gname))
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((batch, net.input.h, net.input.w, net.input.c), device="cuda", generator=gen)
    douts = [torch.randn((batch, t.h, t.w, t.c), device="cuda", generator=gen) for t in net.outputs]
    torch.cuda.synchronize()
    tapes, times = [], []   # (the tapes stay alive to the end: nothing they keep is freed, no address comes back)
    render = Renderer(net)

    def scenario(title, fn):
        t = tape.Tape()
        tape.ACTIVE = t
        t0 = time.perf_counter()
        try:
            fn()
        finally:
            tape.ACTIVE = None
        times.append((title, (time.perf_counter() - t0) * 1e3))
        torch.cuda.synchronize()
        tapes.append((title, t))

    def step():
        net.forward(x, training=True)
        net.backward(douts)

    def infer2():
        net.forward(x, training=False)
        net.forward(x, training=False)

    def changed_step():
        net.mark_params_changed()
        step()

    if batch == 2:
        scenario("1 train step", step)
        scenario("2 train step, planes valid", step)
        scenario("3 mark_params_changed + train step", changed_step)
        scenario("4 inference x2", infer2)
    else:
        scenario("5 inference x2", infer2)
    os.makedirs(outdir, exist_ok=True)
    stem = os.path.join(outdir, f"{gname}__{sname}__b{batch}")
    with open(stem + ".txt", "w") as f:
        for title, t in tapes:
            f.write(f"# scenario {title}: {len(t.entries)} entries\n")
            for line in render.lines(t):
                f.write(line + "\n")
    with open(stem + ".host_ms", "w") as f:     # host time of the eager pass: not part of the comparison
        for title, ms in times:
            f.write(f"{title}: {ms:.1f}\n")


def main(outdir):
    for gname in GRAPHS:
        for sname, env in SETTINGS.items():
            for batch in (2, 1):
                e = {k: v for k, v in os.environ.items() if not k.startswith("YOLO_")}
                e.update(env)
                rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__),
                                     outdir, "child", gname, sname, str(batch)], env=e).returncode
                print(f"{gname} {sname} b{batch}: rc {rc}", flush=True)
                if rc != 0:
                    return rc
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 6 and sys.argv[2] == "child":
        child(sys.argv[1], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    elif len(sys.argv) == 2:
        sys.exit(main(sys.argv[1]))
    else:
        sys.exit(__doc__)
