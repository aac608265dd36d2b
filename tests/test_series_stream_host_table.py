"""What the Python host side of the streaming step and of the bfloat16 series Function does for a grid of calls, against what it did
before that host side was rebuilt from shared helpers (tests/golden/series_stream_host_calls.json, written by
`tools/make_golden.py --series-stream-host-calls` from the code as it stood then -- never regenerated from later code).  The second half
of tests/test_series_host_table.py, whose recorder and stubs it imports.

CPU only.  A streaming row is a SEQUENCE of chunks on one state through one of the five streaming entries (the two forward_stream methods,
tgcn_amd.cheb_stream_relu_pool, F.cheb_time_stream, F.cheb_time_stream_relu_pool); a step of the sequence is a chunk length, optionally
with the call that takes it ("plain", "pool" or "fused": steps of the three kinds alternate on one state), or "reset".  After each chunk
the row records the output's shape and dtype, every logged call with its scalars and null pointers, the ring's shape and dtype, and --
for a host-head state -- (head, seen); a refusal ends the row with its text and whatever was logged before it.  A row's faults (a chunk or
weight of another shape, another state, keywords, grad mode, a capturing stream, other graph arguments) apply to its LAST step, behind
steps that made a good state.  A bfloat16 series row is one call of forward_series / F.cheb_time_windows with bfloat16 parameters,
backward included where the row trains.

The grid: a valid base per entry, varied block by block over dtype, channels and rank, taps, dilation, window step, capturable, fused
(the plan accepting, refusing, and "auto" with the threshold patched high), pool, operand, layer class and bias, then FAULTS one at a
time and in pairs.  Equal chunk results are stored once, and so is every call string."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, _Op
from test_series_host_table import BF, EI, GEOMETRIES, K, N, S, _TableRecorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "series_stream_host_calls.json")
EI2 = torch.tensor([[0, 2], [2, 0]])
METHODS = ("H.forward_stream", "conv.forward_stream")
STREAM = METHODS + ("nn.stream_relu_pool", "F.stream", "F.stream_relu_pool")
SERIES = ("nn.series_bf16", "F.series_bf16")
ENTRIES = STREAM + SERIES
# what a row's spec may hold beside its entry, with the value that the key leaves out
DEFAULTS = dict(layer="H", f=4, dim4=False, H=3, dil=1, stride=1, cap=False, fused=False, pool=4, op="plain", bf16=False, bias=True, plan="ok",
                auto="shipped", steps=None, geom="default", as_series=False, train="no", T=20, chunk=None, weight=None, state=None,
                grad=None, capturing=False, edge_weight=None, graph_args=None, kw={})


def key_of(spec):
    """the row's readable name: the entry, then every setting that is not the default"""
    parts = [spec["entry"]]
    for k in DEFAULTS:
        v = spec.get(k, DEFAULTS[k])
        if k == "kw":
            parts += ["%s=%r" % (a, b) for a, b in sorted(v.items())]
        elif k == "graph_args" and v is not None:
            parts.append("graph_args:%d%s" % (len(v), "other" if len(v) == 1 and v[0] is EI2 else ""))
        elif v != DEFAULTS[k]:
            parts.append("%s:%s" % (k, v))
    return " ".join(parts)


def _steps(spec):
    """Tc = 5, 1, 4 on a host-head state (a window step of 2 or 3 then has a chunk with no window), whole steps on a capturable one"""
    if spec["steps"] is not None:
        return spec["steps"]
    if spec["cap"]:
        return (6, 2, 6) if spec["stride"] == 2 else (6, 3, 6)
    return (5, 1, 4)


STREAM_FAULTS = [
    # the parameters
    dict(bf16=True), dict(bf16="parameters"), dict(bf16="mixed"), dict(bf16="f64"),
    # fused=
    dict(kw=dict(fused="yes")), dict(kw=dict(fused=1)), dict(bf16=True, fused=True), dict(H=1, fused=True), dict(stride=2, fused=True),
    dict(stride=2, fused="auto"), dict(op="nonsquare", fused=True), dict(op="nonsquare"), dict(plan="refuses", fused=True),
    # rank and channels
    dict(chunk=(S, N_V)), dict(chunk=(S, N_V, 4, 4, 1)), dict(f=1, chunk=(S, N_V, 4, 2)), dict(chunk=(S, N_V, 4, 3)), dict(weight=(K, 3, N)),
    dict(weight=(K, 3, 3, N)), dict(f=1, weight=(K, 3, 1, N)), dict(chunk=(S, N_V, 0, 4)),
    # dilation and window step
    dict(kw=dict(dilation=0)), dict(kw=dict(dilation=1.5)), dict(kw=dict(stride=0)), dict(kw=dict(stride=1.5)), dict(dil=2, stride=2),
    dict(kw=dict(dilation=2, stride=2)), dict(cap=True, stride=2, steps=(6, 3)), dict(cap=True, stride=3, steps=(6, 4)),
    # grad mode
    dict(grad="chunk"), dict(grad="on"),
    # the state
    dict(state="not_a_state"), dict(state="dtype"), dict(state="dilation"), dict(state="stride"), dict(state="shape"), dict(state="other_op"),
    dict(kw=dict(dilation=2)), dict(kw=dict(stride=2)), dict(kw=dict(capturable=True)), dict(layer="conv", graph_args=(EI2,)),
    dict(capturing=True), dict(capturing=True, cap=True), dict(capturing=True, H=1),
    # the pool
    dict(kw=dict(pool=3)), dict(kw=dict(pool=8)), dict(kw=dict(pool=True)), dict(chunk=(S, 62, 4, 4)), dict(chunk=(S, 62, 4, 4), steps=(4,)),
    dict(pool=2, chunk=(S, 63, 4, 4), steps=(4,)),
    # the wrapper's own
    dict(layer="other"), dict(graph_args=(EI,)), dict(layer="conv", graph_args=()), dict(layer="conv", graph_args=(EI, None, None)),
    dict(layer="conv", edge_weight="learnable"), dict(layer="conv", edge_weight="fixed"), dict(layer="conv", edge_weight="learnable", bf16=True),
    # pairs: which refusal wins
    dict(bf16=True, kw=dict(pool=3)), dict(kw=dict(pool=3, dilation=0)), dict(chunk=(S, N_V), kw=dict(pool=8)), dict(state="other_op", kw=dict(dilation=0)),
    dict(state="dtype", grad="chunk"), dict(kw=dict(fused="yes", stride=0)), dict(fused=True, bf16=True, H=1), dict(op="nonsquare", fused=True, plan="refuses"),
    dict(state="other_op", fused=True, plan="refuses"), dict(grad="chunk", capturing=True), dict(layer="other", kw=dict(pool=3)),
    dict(layer="conv", edge_weight="learnable", kw=dict(pool=3)), dict(chunk=(S, N_V, 4, 3), kw=dict(dilation=0)), dict(state="shape", capturing=True),
    dict(bf16="mixed", kw=dict(fused="yes")), dict(state="not_a_state", kw=dict(stride=0)),
]

SERIES_FAULTS = [
    dict(f=1), dict(f=1, dim4=True), dict(bf16="parameters"), dict(bf16="mixed"), dict(bf16="f64"), dict(f=1, bf16="parameters"),
    dict(chunk=(S, N_V)), dict(chunk=(S, N_V, 20, 4, 1)), dict(chunk=(S, N_V, 20, 3)), dict(f=1, chunk=(S, N_V, 20, 2)), dict(weight=(K, 3, N)),
    dict(weight=(K, 3, 3, N)), dict(chunk=(S, N_V, 2, 4)), dict(chunk=(S, N_V, 4, 4), kw=dict(dilation=2)),
    dict(kw=dict(padding=3)), dict(kw=dict(padding="same")), dict(kw=dict(padding=(0, 3))), dict(kw=dict(padding=5, dilation=2)),
    dict(kw=dict(stride=0)), dict(kw=dict(stride=1.5)), dict(kw=dict(dilation=0)), dict(kw=dict(dilation=2, stride=2)), dict(kw=dict(dilation=40)),
    dict(kw=dict(time_chunk=6, padding="causal")), dict(kw=dict(time_chunk=0)), dict(kw=dict(fused=True)), dict(kw=dict(fused="auto")),
    dict(kw=dict(fused="yes")), dict(layer="conv", edge_weight="learnable"), dict(layer="conv", edge_weight="fixed"),
    # pairs
    dict(f=1, kw=dict(padding=3)), dict(bf16="parameters", kw=dict(stride=0)), dict(kw=dict(fused=True, time_chunk=6, padding="causal")),
    dict(f=1, kw=dict(fused=True)), dict(bf16="mixed", kw=dict(fused="yes")), dict(chunk=(S, N_V, 20, 3), kw=dict(padding=3)),
]


def grid():
    """the specs of every row, in a fixed order, each key once"""
    rows, seen = [], set()

    def add(entry, **spec):
        kw = spec.get("kw", {})
        pooled, method, fn = "relu_pool" in entry, entry in METHODS, entry.startswith("F.")
        steps = spec.get("steps") or ()
        if entry in METHODS:
            if spec.get("layer", "H") not in ("H", entry[:entry.index(".")]):
                return      # a method has its own class
            spec = dict(spec, layer="H")
        if fn and (spec.get("edge_weight") or spec.get("graph_args") is not None or spec.get("layer") == "other"):
            return          # the wrappers' own checks
        if not fn and (spec.get("weight") is not None or spec.get("op") == "nonsquare"):
            return          # only the functions take a weight or an operand from the caller
        if spec.get("op") == "nonsquare" and spec.get("fused") is not True:
            return          # only fused=True looks at the operand's shape
        if method and spec.get("graph_args") is not None and not (len(spec["graph_args"]) == 1 and entry == "conv.forward_stream"):
            return          # a method: Python's own TypeError
        if entry in STREAM:
            if pooled and (spec.get("stride", 1) != 1 or spec.get("fused", False) is not False or "fused" in kw or "stride" in kw
                           or any(isinstance(s, tuple) and s[1] == "fused" for s in steps)):
                return      # no fused= and no stride=
            if not pooled and ("pool" in kw or (spec.get("chunk") or (S, N_V))[1] != N_V):
                return      # only the pool looks at the vertex count
        spec = dict(spec, entry=entry)
        if key_of(spec) not in seen:
            seen.add(key_of(spec))
            rows.append(spec)

    shapes = (dict(f=1), dict(f=1, dim4=True), dict(f=3), dict(f=4), dict(f=8))
    for entry in STREAM:
        pooled = "relu_pool" in entry
        classes = ("H",) if entry in METHODS else ("H", "conv")
        # dtype x channels and rank x taps x capturable
        for bf16 in ((False,) if pooled else (False, True)):
            for shape in shapes:
                for H in (1, 3):
                    for cap in (False, True):
                        add(entry, bf16=bf16, H=H, cap=cap, **shape)
        # dilation and window step
        for bf16 in ((False,) if pooled else (False, True)):
            for dil, stride in ((2, 1), (1, 2), (1, 3)):
                for H in (1, 3):
                    for cap in (False, True):
                        add(entry, bf16=bf16, H=H, cap=cap, dil=dil, stride=stride, f=(3 if bf16 else 4))
        # the layer class, the pool, the bias
        for layer in classes:
            for pool in (2, 4):
                for H in (1, 3):
                    for cap in (False, True):
                        add(entry, layer=layer, pool=pool, H=H, cap=cap)
            add(entry, layer=layer, bias=False)
            add(entry, layer=layer, bias=False, f=1, cap=True)
        # the one-launch step: asked for, left to the rule (as shipped and with the threshold high), a plan that refuses
        for fused in (True, "auto"):
            for plan in ("ok", "refuses"):
                for auto in ("shipped", "high"):
                    for cap in (False, True):
                        add(entry, fused=fused, plan=plan, auto=auto, cap=cap)
            add(entry, fused=fused, dil=2, f=1)
        add(entry, fused="auto", auto="high", H=1)
        add(entry, fused="auto", auto="high", bf16=True)
        add(entry, fused="auto", auto="high", stride=2)
        add(entry, fused="auto", auto="high", steps=(5, 40))
        # the operand
        for op in ("reordered", "nonsquare"):
            for cap in (False, True):
                add(entry, op=op, cap=cap)
                add(entry, op=op, cap=cap, layer="conv", pool=2, H=1)
            add(entry, op=op, stride=2)
            add(entry, op=op, bf16=True, f=3)
            add(entry, op=op, fused=True)
            add(entry, op=op, fused="auto", auto="high")
        # pooled, unpooled and fused steps alternate on one state; a reset in the middle
        for layer in classes:
            for cap in (False, True):
                add(entry, layer=layer, cap=cap, dil=2, steps=((5, "plain"), (1, "pool"), (4, "fused"), (3, "pool"), (2, "plain")))
                add(entry, layer=layer, cap=cap, steps=(5, 1, "reset", 4, 3))
            add(entry, layer=layer, steps=((3, "pool"), (3, "fused"), "reset", (5, "plain")), op="reordered")
            add(entry, layer=layer, H=1, cap=True, steps=((3, "pool"), (2, "plain"), (4, "pool")))
        add(entry, stride=2, steps=(1, 1, 1, "reset", 2, 1))
        add(entry, stride=3, bf16=True, steps=(1, 1, 1, 1, 7))
        for i, fault in enumerate(STREAM_FAULTS):
            for layer in (classes if i < 4 else ("H",)):
                add(entry, **dict(fault, layer=fault.get("layer", layer), steps=fault.get("steps", (5, 4))))
    for entry in SERIES:
        # geometry x layout x what trains
        for geom in GEOMETRIES:
            for as_series in (False, True):
                for train in ("no", "all", "frozen", "series"):
                    add(entry, bf16=True, geom=geom, as_series=as_series, train=train)
        # channels, with T*f a multiple of 8 and not
        for f in (1, 3, 4, 8):
            for T in (21, 24):
                for train in ("no", "all"):
                    add(entry, bf16=True, f=f, T=T, as_series=True, train=train)
                add(entry, bf16=True, f=f, T=T, geom="dilated", layer="conv", train="all")
        # the operand, the layer class, the bias
        for geom in ("default", "causal", "dilated", "stride2"):
            for train in ("no", "all", "series"):
                add(entry, bf16=True, geom=geom, op="reordered", train=train, as_series=(geom != "causal"))
            add(entry, bf16=True, geom=geom, layer="conv", train="all", f=3)
            add(entry, bf16=True, geom=geom, bias=False, train="all")
        add(entry, bf16=True, f=1, dim4=True, as_series=True, train="all")
        add(entry, bf16=True, f=1, geom="causal", layer="conv", train="all")
        for i, fault in enumerate(SERIES_FAULTS):
            for layer in (("H", "conv") if i < 6 else ("H",)):
                add(entry, **dict(dict(bf16=True), **dict(fault, layer=fault.get("layer", layer))))
    return rows


class _StreamRecorder(_TableRecorder):
    """the table's recorder; refuse=True answers TGCN_ERR_UNSUPPORTED to the one-launch step's plan too, and logs that it was asked"""

    def __getattr__(self, name):
        if name == "tgcn_cheb_stream_small_plan" and self.refuse:
            def plan(*args):
                self.note("(cheb_stream_small_plan refuses)")
                return -4
            return plan
        return super().__getattr__(name)


def _dtypes(spec):
    """(the input's dtype, the weight's, the bias') of a row"""
    return {False: (torch.float32,) * 3, True: (BF,) * 3, "parameters": (torch.float32, BF, BF), "mixed": (BF, BF, torch.float32),
            "f64": (torch.float32, torch.float64, torch.float64)}[spec["bf16"]]


def _layer(spec):
    """(the module of an nn row, its graph arguments)"""
    f, H = spec["f"], spec["H"]
    kind = spec["entry"][:spec["entry"].index(".")] if spec["entry"] in METHODS else spec["layer"]
    if kind == "other":
        layer, extra = tgcn_amd.GCNCheb(torch.eye(N_V), f, N, K, bias=spec["bias"]), ()
    elif kind == "H":
        layer, extra = tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, N, K, H, bias=spec["bias"]), ()
    else:
        layer, extra = tgcn_amd.ChebTimeConv(f, N, K, H, bias=spec["bias"]), (EI,)
        if spec["edge_weight"]:
            extra += (torch.ones(2, requires_grad=spec["edge_weight"] == "learnable"),)
    _, wd, bd = _dtypes(spec)
    layer = layer.to(wd)
    if bd != wd and layer.bias is not None:
        layer.bias.data = layer.bias.data.to(bd)
    return layer, extra


def _parameters(spec, rank3, weight=None):
    """(weight, bias, bias_kind, mode) of an F row"""
    _, wd, bd = _dtypes(spec)
    W = torch.zeros(weight or ((K, spec["H"], N) if rank3 else (K, spec["H"], spec["f"], N)), dtype=wd)
    if not spec["bias"]:
        return W, None, F.BIAS_NONE, F.MODE_POWER if spec["layer"] == "H" else F.MODE_CHEBYSHEV
    if spec["layer"] == "H":
        return W, torch.zeros(N_V * N, dtype=bd), F.BIAS_VERTEX_CHANNEL, F.MODE_POWER
    return W, torch.zeros(N, dtype=bd), F.BIAS_CHANNEL, F.MODE_CHEBYSHEV


def _other_state(kind, st):
    """the state of a row's last step: the recording's own with one thing changed"""
    if kind == "not_a_state":
        return "state"
    a = dict(op=st.op, dtype=st.dtype, S=st.S, n=st.n, f=st.f, K=st.K, H=st.H, dilation=st.dilation, device="cpu", capturable=st.capturable,
             stride=st.stride)
    a.update({"other_op": dict(op=_Op(N_V, 256)), "dtype": dict(dtype=BF if st.dtype != BF else torch.float32),
              "dilation": dict(dilation=st.dilation + 1), "stride": dict(stride=st.stride + 1), "shape": dict(S=st.S + 1)}[kind])
    return F.SeriesStreamState(**a)


def _operand(spec):
    return {"plain": _Op(N_V, 256), "reordered": _Op(N_V, 256, perm=True), "nonsquare": _Op(N_V, 256, n_cols=N_V + 1)}[spec["op"]]


def _run_stream(spec, mp, rec, reads, count):
    entry, f = spec["entry"], spec["f"]
    fn = entry.startswith("F.")
    if fn:
        op = _operand(spec)
    else:
        layer, extra = _layer(spec)
    steps, state, rows = _steps(spec), None, []
    for i, step in enumerate(steps):
        if step == "reset":
            state.reset()
            continue
        Tc, how = step if isinstance(step, tuple) else (step, "pool" if "relu_pool" in entry else "plain")
        last = i == len(steps) - 1
        kw = dict(dilation=spec["dil"], capturable=spec["cap"], state=state)
        if how == "pool":
            kw["pool"] = spec["pool"]
        else:
            kw.update(fused=True if how == "fused" else spec["fused"], stride=spec["stride"])
        shape = (S, N_V, Tc) if f == 1 and not spec["dim4"] else (S, N_V, Tc, f)
        weight, graph_args, grad = None, None, None
        if last:
            shape, weight, graph_args, grad = spec["chunk"] or shape, spec["weight"], spec["graph_args"], spec["grad"]
            kw.update(spec["kw"])
            if spec["state"]:
                kw["state"] = _other_state(spec["state"], state)
            if spec["capturing"]:
                mp.setattr(F, "stream_is_capturing", lambda: True)
        chunk = torch.zeros(shape, dtype=_dtypes(spec)[0])
        if grad == "chunk":
            chunk.requires_grad_(True)
        if fn:
            W, bias, bias_kind, mode = _parameters(spec, len(shape) == 3, weight)
            if how == "pool":
                call = lambda: F.cheb_time_stream_relu_pool(op, chunk, W, bias, bias_kind, mode, kw.pop("pool"), **kw)
            else:
                call = lambda: F.cheb_time_stream(op, chunk, W, bias, bias_kind, mode, **kw)
        else:
            args = extra if graph_args is None else graph_args
            if how == "pool":
                call = lambda: tgcn_amd.cheb_stream_relu_pool(layer, chunk, *args, **kw)
            else:
                call = lambda: layer.forward_stream(chunk, *args, **kw)
        del rec.calls[:], rec.nulls[:]
        count[0] = 0
        try:
            with (torch.enable_grad() if grad else torch.no_grad()):
                out, state = call()
        except _lib.TgcnError as e:
            rows.append({"error": str(e), "calls": list(rec.calls)})
            break
        row = {"shape": list(out.shape), "dtype": str(out.dtype), "calls": list(rec.calls), "nulls": [list(n) for n in rec.nulls],
               "ring": None if state.ring is None else [list(state.ring.shape), str(state.ring.dtype)]}
        if state.capturable:
            reads.append((key_of(spec), i, count[0]))
        else:
            row["position"] = [state.head, state.seen]
        rows.append(row)
    return rows


def _run_series(spec, rec):
    entry, f = spec["entry"], spec["f"]
    shape = spec["chunk"] or ((S, N_V, spec["T"]) if f == 1 and not spec["dim4"] else (S, N_V, spec["T"], f))
    series = torch.zeros(shape, dtype=_dtypes(spec)[0])
    kw = dict(GEOMETRIES[spec["geom"]], as_series=spec["as_series"])
    kw.update(spec["kw"])
    if entry.startswith("F."):
        W, bias, bias_kind, mode = _parameters(spec, len(shape) == 3, spec["weight"])
        op = _operand(spec)
        leaves, call = (series, W, bias), lambda: F.cheb_time_windows(op, series, W, bias, bias_kind, mode, **kw)
    else:
        layer, extra = _layer(spec)
        leaves, call = (series, layer.weight, layer.bias), lambda: layer.forward_series(series, *extra, **kw)
    train = spec["train"]
    needs = {"no": (0, 0, 0), "all": (1, 1, 1), "frozen": (1, 0, 1), "series": (1, 0, 0)}[train]
    for t, need in zip(leaves, needs):
        if t is not None:
            t.requires_grad_(bool(need))
    try:
        with (torch.enable_grad() if train != "no" else torch.no_grad()):
            z = call()
            if train != "no":
                z.backward(torch.ones_like(z))
    except _lib.TgcnError as e:
        return [{"error": str(e), "calls": list(rec.calls)}]
    return [{"shape": list(z.shape), "dtype": str(z.dtype), "calls": list(rec.calls), "nulls": [list(n) for n in rec.nulls]}]


def run(spec, reads=None):
    """one row's results, a list with one of them per chunk: {"error", "calls"} of a refused call (the row's last), {"shape", "dtype",
    "calls", "nulls"[, "ring", "position"]} of an accepted one.  reads collects (row, step, how often SeriesStreamState.head and .seen
    were read during the call) of every accepted call on a capturable state."""
    spec = dict(DEFAULTS, **spec)
    reads = [] if reads is None else reads
    with pytest.MonkeyPatch.context() as mp:
        rec = _StreamRecorder(spec["plan"] == "refuses")
        mp.setattr(_lib, "lib", lambda: rec)
        mp.setattr(_lib, "require_device", lambda *t: None)
        mp.setattr(_lib, "stream_ptr", lambda: ctypes.c_void_p(0))
        mp.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
        mp.setattr(torch.cuda, "mem_get_info", lambda d=None: (1 << 34, 1 << 35))

        def built(*a, **k):
            rec.note("(operand built)")
            return _Op(N_V, 256, perm=spec["op"] == "reordered")
        mp.setattr(GraphOperand, "from_any", staticmethod(built))
        mp.setattr(GraphOperand, "from_edge_index", staticmethod(built))
        if spec["auto"] == "high":
            mp.setattr(F, "STREAM_FUSED_AUTO_MAX_TC", 8)
        count = [0]
        head, seen = F.SeriesStreamState.head, F.SeriesStreamState.seen

        def counted(prop):
            def get(self):
                count[0] += 1
                return prop.fget(self)
            return property(get)
        mp.setattr(F.SeriesStreamState, "head", counted(head))
        mp.setattr(F.SeriesStreamState, "seen", counted(seen))
        if spec["entry"] in SERIES:
            return _run_series(spec, rec)
        return _run_stream(spec, mp, rec, reads, count)


def table():
    """{"rows": {key: [index into results, one per chunk]}, "results": [...], "calls": [...]}: rows in the grid's order, equal chunk
    results stored once, their "calls" as indices into the list of distinct call strings"""
    rows, results, index, calls, cindex = {}, [], {}, [], {}
    for spec in grid():
        rows[key_of(spec)] = ids = []
        for res in run(spec):
            res = dict(res, calls=[cindex.setdefault(c, len(cindex)) for c in res["calls"]])
            text = json.dumps(res, sort_keys=True)
            if text not in index:
                index[text] = len(results)
                results.append(json.loads(text))
            ids.append(index[text])
    calls = sorted(cindex, key=cindex.get)
    return {"rows": rows, "results": results, "calls": calls}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def _then(recorded, key):
    """a recorded row with its call strings spelled out"""
    return [dict(recorded["results"][i], calls=[recorded["calls"][c] for c in recorded["results"][i]["calls"]]) for i in recorded["rows"][key]]


def test_every_row_does_what_the_recording_did(recorded):
    specs = grid()
    assert [key_of(s) for s in specs] == list(recorded["rows"])
    wrong = []
    for spec in specs:
        now, then = run(spec), _then(recorded, key_of(spec))
        if now != then:
            wrong.append((key_of(spec), now, then))
    assert not wrong, "%d rows differ; (row, now, recorded) of the first: %s" % (len(wrong), wrong[:3])


def test_a_capturable_state_is_never_read_on_the_host_during_a_call():
    """SeriesStreamState.head and .seen synchronise on a capturable state, and a read inside a capture fails: no accepted call reads them"""
    reads = []
    for spec in grid():
        if spec["entry"] in STREAM:
            run(spec, reads)
    assert len(reads) >= 100 and not [r for r in reads if r[2]], [r for r in reads if r[2]][:5]


# a fragment of every refusal that stream_precheck, _stream_args, _state_operand_check, cheb_stream_relu_pool, check_series_bf16 and the
# two cheb_time_stream* functions document (and of series_geometry's, which they pass on)
REFUSALS = [
    "parameters of dtype", "-- convert both (module.to(dtype))", "fused is False, True or \"auto\"", "fused=True runs in float32 only",
    "fused=True needs a ring", "a (S, n, Tc) chunk takes a (K, H, N) weight", "channels, the weight", "a chunk holds at least one time row",
    "dilation is an integer >= 1", "stride is an integer >= 1", "together with stride", "fused=True has no window step",
    "the parameters are bfloat16 but the chunk is", "streaming has no backward", "state is a SeriesStreamState or None",
    "the state was made for dtype", "the state was made for dilation", "the state was made for stride", "the state was made for (S, n, f, K, H)",
    "capturable=True with a state that keeps its head on the host", "takes chunks of whole steps", "the stream is capturing a hipGraph",
    "the chunk is (S, n, Tc) or (S, n, Tc, f)", "channel(s), the layer in_channels", "a graph this layer's operand cache no longer holds",
    "the state was made for another operand -- one state per layer and graph", "fused=True needs a square operand",
    "do not fit the one-launch step", "the layer is a TGCNCheb_H or a ChebTimeConv", "after the series", "bfloat16 parameters are not supported",
    "learnable edge weights", "streaming is inference only; detach() the weight", "pool is 2 or 4", "are not a multiple of pool",
    "the scalar-load form", "the parameters are bfloat16 but the series is", "time_chunk runs in float32 only",
]


def test_the_recording_is_small_and_covers_both_blocks(recorded):
    rows, results = recorded["rows"], recorded["results"]
    assert len(rows) <= 1000 and os.path.getsize(GOLDEN) < 256 * 1024
    assert sorted({i for ids in rows.values() for i in ids}) == list(range(len(results)))
    assert sorted({c for r in results for c in r["calls"]}) == list(range(len(recorded["calls"])))
    refused = sum("error" in results[ids[-1]] for ids in rows.values())
    assert len(rows) - refused >= 0.4 * len(rows), (refused, len(rows))
    errors = {(key.split()[0], results[ids[-1]]["error"]) for key, ids in rows.items() if "error" in results[ids[-1]]}
    for entry in ENTRIES:
        assert any("shape" in results[i] and results[i]["calls"] for key, ids in rows.items() if key.split()[0] == entry for i in ids), entry
        assert sum(e == entry for e, _ in errors) >= 10, entry
    for text in REFUSALS:
        assert any(text in msg for _, msg in errors), text
    # a host-head sequence at a window step in which a chunk returns no window, and capturable sequences of whole steps
    assert any("shape" in results[i] and results[i]["shape"][2] == 0 and "position" in results[i] for ids in rows.values() for i in ids)
    assert any("shape" in results[i] and "position" not in results[i] and "ring" in results[i] for ids in rows.values() for i in ids)
