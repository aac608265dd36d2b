"""What the Python host side of the float32 time-window family does for a grid of calls, against what it did before that host side was
rebuilt from shared helpers (tests/golden/series_host_calls.json, written by `tools/make_golden.py --series-host-calls` from the code
as it stood then -- never regenerated from later code).  It does for tgcn_amd/functional.py and tgcn_amd/nn.py what
tests/test_series_refusal_table.py does for the C entries.

CPU only, by the recorder of tests/test_layer_dispatch.py: `_lib.lib` is a recorder, operands are stubs.  A row is one call of one of
the ten entries (the four tgcn_amd.cheb_series_relu_* wrappers and forward_series, the four F.cheb_time_windows_relu_* functions and
F.cheb_time_windows) and records either the TgcnError's text with whatever had been logged before it, or the output's shape, every
logged launch with its scalars (the backward's too where the row trains) and the positions of the null pointers.  A built operand and
a refused plan are logged as calls of their own, so "before an operand is built" is part of the record.

The grid: one valid base call per entry (S=2, n=N_V, T=20, K=3, H=3, N=8, pool=4), varied block by block over the axes that pick a
path -- channels and series rank, layer class, layout, what trains, plain / reordered operand, geometry, p / training, time_chunk,
fused and a plan that refuses -- then FAULTS: one argument moved at a time through every refusal the entries document, and a few pairs
that pin which refusal wins.  A row's key spells its call out; rows with equal results share one stored result."""
import ctypes
import contextlib
import json
import os

import pytest
import torch

import tgcn_amd
from tgcn_amd import _lib
from tgcn_amd import functional as F
from tgcn_amd.graph import GraphOperand

from test_layer_dispatch import N_V, _Op, _Recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "series_host_calls.json")
S, T, K, H, N = 2, 20, 3, 3, 8
BF = torch.bfloat16
EI = torch.tensor([[0, 1], [1, 0]])
GEOMETRIES = {"default": {}, "causal": dict(padding="causal"), "dilated": dict(padding=(1, 3), dilation=2), "stride2": dict(stride=2),
              "dil2": dict(dilation=2), "causal-dil2": dict(padding="causal", dilation=2)}
_CONV = ("default", "causal", "dilated", "stride2")
_POOLED = ("pool", "as_series", "padding", "dilation")

# entry -> (function name, the keywords it takes, the base call's keywords, its geometries)
ENTRIES = {
    "nn.relu_pool": ("cheb_series_relu_pool", _POOLED + ("stride",), dict(pool=4), _CONV),
    "nn.relu_dropout_pool": ("cheb_series_relu_dropout_pool", _POOLED + ("stride", "p", "seed", "training"), dict(pool=4, p=0.5, seed=7), _CONV),
    "nn.relu_pool_chunked": ("cheb_series_relu_pool_chunked", ("pool", "as_series", "dilation", "p", "seed", "training", "time_chunk"),
                             dict(pool=4, time_chunk=40), ("default", "dil2")),
    "nn.relu_pool_fused": ("cheb_series_relu_pool_fused", _POOLED + ("p", "seed", "training", "fused"), dict(pool=4), _CONV[:3]),
    "nn.forward_series": ("forward_series", ("as_series", "stride", "padding", "dilation", "time_chunk", "fused"), {}, _CONV),
    "F.relu_pool": ("cheb_time_windows_relu_pool", _POOLED + ("stride",), dict(pool=4), _CONV),
    "F.relu_dropout_pool": ("cheb_time_windows_relu_dropout_pool", _POOLED + ("stride", "p", "seed"), dict(pool=4, p=0.5, seed=7), _CONV),
    "F.relu_pool_chunked": ("cheb_time_windows_relu_pool_chunked", ("pool", "as_series", "dilation", "p", "seed", "time_chunk"),
                            dict(pool=4, time_chunk=40), ("default", "dil2")),
    "F.relu_pool_fused": ("cheb_time_windows_relu_pool_fused", _POOLED + ("p", "seed", "fused"), dict(pool=4), _CONV[:3]),
    "F.cheb_time_windows": ("cheb_time_windows", ("as_series", "stride", "padding", "dilation", "time_chunk", "fused"), {}, _CONV),
}
# what a row's spec may hold beside its entry, with the value that the key leaves out
DEFAULTS = dict(layer="H", f=4, dim4=False, as_series=False, train="no", op="plain", geom="default", plan="ok", auto="shipped", kw={},
                bf16=False, series=None, weight=None, edge_weight=None, graph_args=None)
TRAIN = ("no", "all", "frozen")       # no grad / series, weight and bias train / the weight is frozen


def key_of(spec):
    """the row's readable name: the entry, then every setting that is not the default"""
    parts = [spec["entry"]]
    for k in DEFAULTS:
        v = spec.get(k, DEFAULTS[k])
        if k == "kw":
            parts += ["%s=%s" % (a, "tensor%s" % (tuple(b.shape),) if isinstance(b, torch.Tensor) else repr(b)) for a, b in sorted(v.items())]
        elif v != DEFAULTS[k]:
            parts.append("%s:%s" % (k, v))
    return " ".join(parts)


def grid():
    """the specs of every row, in a fixed order, each key once"""
    rows, seen = [], set()

    def add(entry, **spec):
        kw = spec.get("kw", {})
        if any(k not in ENTRIES[entry][1] for k in kw):
            return          # the entry has no such keyword
        if entry.startswith("F.") and (spec.get("edge_weight") or spec.get("graph_args") is not None or spec.get("layer") == "other"):
            return          # the wrappers' own checks
        if entry.startswith("nn.") and (spec.get("weight") is not None or spec.get("op") == "nonsquare" or spec.get("dim4")):
            return          # only the functions take a weight or an operand from the caller
        if entry == "nn.forward_series" and (spec.get("graph_args") is not None or spec.get("layer") == "other"):
            return          # a method: Python's own TypeError / AttributeError
        if spec.get("op") == "nonsquare" and kw.get("fused", entry == "F.relu_pool_fused") is not True:
            return          # only fused=True looks at the operand's shape
        if "pool" not in ENTRIES[entry][1] and (spec.get("series") or (S, N_V))[1] != N_V:
            return          # only the pool refuses another vertex count
        spec = dict(spec, entry=entry)
        if key_of(spec) not in seen:
            seen.add(key_of(spec))
            rows.append(spec)

    for entry, (_, takes, base, geoms) in ENTRIES.items():
        ring = ("causal", "causal-dil2") if "padding" in takes else geoms         # the geometries a time_chunk runs at
        # channels and rank x layer class x layout (x training, window-major)
        for shape in (dict(f=4), dict(f=1), dict(f=1, dim4=True)):
            for layer in ("H", "conv"):
                for as_series, train in ((False, "no"), (True, "no"), (False, "all"))[:3 if layer == "H" else 1]:
                    add(entry, layer=layer, as_series=as_series, train=train, **shape)
        # geometry x operand x what trains
        for geom in geoms:
            for op in ("plain", "reordered"):
                for train in (TRAIN if op == "plain" else ("no", "all")):
                    add(entry, geom=geom, op=op, train=train, as_series=(geom != "default"))
        add(entry, geom=geoms[1], layer="conv", f=1, train="all")
        add(entry, layer="conv", train="all")
        # the mask
        if "p" in takes:
            for p in (0, 0.5):
                for op in ("plain", "reordered"):
                    for train in ("no", "all"):
                        add(entry, op=op, train=train, kw=dict(p=p, seed=7))
            add(entry, kw=dict(p=0.5, seed=None))
            add(entry, kw=dict(p=0.5, seed=torch.zeros(1, dtype=torch.int64)), train="all")
            add(entry, kw=dict(p=0.5, seed=7, training=False), train="all")
            add(entry, kw=dict(p=0.5, seed=7, training=False), op="reordered")
            add(entry, geom=geoms[1], as_series=True, layer="conv", train="frozen", kw=dict(p=0.5, seed=7))
        # time chunks: four of them, and one that holds the whole recording
        if "time_chunk" in takes:
            for train in TRAIN:
                add(entry, geom=ring[0], train=train, kw=dict(time_chunk=6))
                add(entry, geom=ring[0], train=train, kw=dict(time_chunk=40))
                add(entry, geom=ring[1], as_series=True, train=train, kw=dict(time_chunk=6))
            for train in ("no", "all"):
                add(entry, geom=ring[0], op="reordered", train=train, kw=dict(time_chunk=6))
            add(entry, geom=ring[1], op="reordered", as_series=True, train="all", kw=dict(time_chunk=40))
            add(entry, geom=ring[0], layer="conv", f=1, train="all", kw=dict(time_chunk=6))
            if "p" in takes:
                add(entry, geom=ring[1], train="all", kw=dict(time_chunk=6, p=0.5, seed=7))
                add(entry, geom=ring[0], op="reordered", train="all", kw=dict(time_chunk=6, p=0.5, seed=7))
                add(entry, geom=ring[0], as_series=True, train="frozen", kw=dict(time_chunk=40, p=0.5, seed=7))
        # the one-launch layer: asked for, left to the rule (as shipped, and with every class listed), and a plan that refuses
        if "fused" in takes:
            for mask in ((dict(), dict(p=0.5, seed=7)) if "p" in takes else (dict(),)):
                for geom in _CONV[:3]:
                    for train in ("no", "all"):
                        add(entry, geom=geom, train=train, as_series=(geom != "default"), kw=dict(mask, fused=True))
                for auto in ("shipped", "all"):
                    add(entry, auto=auto, kw=dict(mask, fused="auto"))
                    add(entry, geom="dilated", as_series=True, train="all", auto=auto, kw=dict(mask, fused="auto"))
                    add(entry, plan="refuses", train="all", auto=auto, kw=dict(mask, fused="auto"))
                add(entry, op="reordered", kw=dict(mask, fused=True))
                add(entry, op="reordered", auto="all", train="all", kw=dict(mask, fused="auto"))
                add(entry, plan="refuses", kw=dict(mask, fused=True))
                add(entry, f=1, layer="conv", train="frozen", kw=dict(mask, fused=True))
            for fused, auto in ((True, "shipped"), ("auto", "shipped"), ("auto", "all")):
                add(entry, f=1, auto=auto, kw=dict(fused=fused))
                add(entry, f=1, dim4=True, train="all", auto=auto, kw=dict(fused=fused))
                add(entry, f=1, as_series=True, auto=auto, kw=dict(fused=fused))
        # the faults, alone and in pairs
        for i, fault in enumerate(FAULTS):
            for layer in (("H", "conv") if i < 2 else ("H",)):       # the first two through both layer classes
                add(entry, **dict(fault, layer=fault.get("layer", layer)))
    return rows


FAULTS = [
    dict(bf16=True), dict(bf16=True, as_series=True), dict(bf16="parameters"), dict(bf16=True, f=1), dict(kw=dict(pool=3)), dict(series=(S, N_V, T, 3)),
    dict(series=(S, 62, T, 4)),
    # rank and channels
    dict(series=(S, N_V)), dict(series=(S, N_V, T, 4, 1)), dict(f=1, series=(S, N_V, T, 2)), dict(weight=(K, H, N)), dict(weight=(K, H, 3, N)),
    dict(f=1, weight=(K, H, 1, N)), dict(series=(S, N_V, 2, 4)), dict(series=(S, N_V, 4, 4), geom="dil2"),
    # the pool
    dict(kw=dict(pool=8)), dict(kw=dict(pool=True)), dict(kw=dict(pool=2)), dict(series=(S, 63, T, 4), kw=dict(pool=2)),
    # the geometry
    dict(kw=dict(padding=3)), dict(kw=dict(padding="same")), dict(kw=dict(padding=(0, 3))),
    dict(kw=dict(padding=5, dilation=2)), dict(kw=dict(stride=0)), dict(kw=dict(stride=1.5)),
    dict(kw=dict(dilation=0)), dict(kw=dict(dilation=2, stride=2)), dict(kw=dict(dilation=40)),
    # the mask
    dict(kw=dict(p=1.0)), dict(kw=dict(p=-0.1)), dict(kw=dict(p=0.5, seed=-1)), dict(kw=dict(p=0.5, seed=2 ** 62)),
    dict(kw=dict(p=0.5, seed=torch.zeros(2, dtype=torch.int64))), dict(kw=dict(p=1.0, training=False)),
    # time chunks
    dict(kw=dict(time_chunk=0)), dict(kw=dict(time_chunk=2.5)), dict(kw=dict(time_chunk=None)),
    dict(kw=dict(time_chunk=6, padding=0)), dict(kw=dict(time_chunk=6, padding="causal", stride=2)),
    dict(kw=dict(time_chunk=6, padding="causal"), bf16=True),
    # fused=
    dict(kw=dict(fused="yes")), dict(kw=dict(fused=False)), dict(kw=dict(fused=True, stride=2)),
    dict(kw=dict(fused=True, time_chunk=6, padding="causal")), dict(kw=dict(fused=True), bf16=True), dict(kw=dict(fused="auto"), bf16=True),
    dict(kw=dict(fused=True), op="nonsquare"), dict(op="nonsquare"),
    # the wrappers' own
    dict(layer="conv", edge_weight="learnable"), dict(layer="conv", edge_weight="fixed"), dict(layer="other"), dict(graph_args=(EI,)),
    dict(layer="conv", graph_args=()), dict(layer="conv", graph_args=(EI, None, None)),
    # pairs: which refusal wins
    dict(bf16=True, kw=dict(pool=3)), dict(kw=dict(pool=3, padding=3)), dict(kw=dict(p=1.0, pool=3)), dict(bf16=True, kw=dict(p=1.0)),
    dict(kw=dict(p=0.5, seed=-1, time_chunk=0)), dict(series=(S, N_V), kw=dict(pool=8)), dict(series=(S, 62, T, 4), kw=dict(padding=3)),
    dict(bf16=True, kw=dict(time_chunk=None)), dict(kw=dict(fused="yes", p=1.0)), dict(layer="conv", edge_weight="learnable", bf16=True),
    dict(op="nonsquare", kw=dict(fused=True, pool=3)), dict(series=(S, N_V, T, 3), kw=dict(pool=3)), dict(weight=(K, H, N), kw=dict(padding=3)),
    dict(layer="other", kw=dict(pool=3)), dict(layer="conv", edge_weight="learnable", kw=dict(p=1.0)), dict(kw=dict(time_chunk=0, pool=3)),
    dict(op="reordered", plan="refuses", kw=dict(fused=True)), dict(kw=dict(stride=0, padding="same")),
    dict(series=(S, N_V, T, 3), kw=dict(fused=True, stride=2)), dict(kw=dict(time_chunk=6, padding=0, fused="yes")),
]


class _TableRecorder(_Recorder):
    """the recorder; refuse=True answers TGCN_ERR_UNSUPPORTED to the one-launch layer's plan, and logs that it was asked"""

    def __init__(self, refuse):
        super().__init__({})
        self.refuse = refuse

    def note(self, what):
        self.calls.append(what)
        self.nulls.append(())

    def __getattr__(self, name):
        if name == "tgcn_cheb_series_small_plan" and self.refuse:
            def plan(*args):
                self.note("(cheb_series_small_plan refuses)")
                return -4
            return plan
        if name == "tgcn_last_error":
            return lambda: b"the recorder refuses"
        return super().__getattr__(name)


def _arguments(spec):
    """(function, positional arguments, the tensors that train) of a row"""
    entry, f = spec["entry"], spec["f"]
    shape = spec["series"] or ((S, N_V, T) if f == 1 and not spec["dim4"] else (S, N_V, T, f))
    series = torch.zeros(shape, dtype=BF if spec["bf16"] is True else torch.float32)
    name = ENTRIES[entry][0]
    if entry.startswith("nn."):
        if spec["layer"] == "other":
            layer, extra = tgcn_amd.GCNCheb(torch.eye(N_V), f, N, K), ()
        elif spec["layer"] == "H":
            layer, extra = tgcn_amd.TGCNCheb_H(torch.eye(N_V), f, N, K, H), ()
        else:
            layer, extra = tgcn_amd.ChebTimeConv(f, N, K, H), (EI,)
            if spec["edge_weight"]:
                extra += (torch.ones(2, requires_grad=spec["edge_weight"] == "learnable"),)
        if spec["graph_args"] is not None:
            extra = spec["graph_args"]
        if spec["bf16"]:
            layer = layer.to(BF)
        if name == "forward_series":
            return getattr(layer, name, None), (series,) + tuple(extra), (series, layer.weight, layer.bias)
        return getattr(tgcn_amd, name), (layer, series) + tuple(extra), (series, layer.weight, layer.bias)
    dt = BF if spec["bf16"] else torch.float32
    weight = torch.zeros(spec["weight"] or ((K, H, N) if len(shape) == 3 else (K, H, f, N)), dtype=dt)
    bias, bias_kind, mode = ((torch.zeros(N_V * N, dtype=dt), F.BIAS_VERTEX_CHANNEL, F.MODE_POWER) if spec["layer"] == "H" else
                             (torch.zeros(N, dtype=dt), F.BIAS_CHANNEL, F.MODE_CHEBYSHEV))
    op = {"plain": _Op(N_V, 256), "reordered": _Op(N_V, 256, perm=True), "nonsquare": _Op(N_V, 256, n_cols=N_V + 1)}[spec["op"]]
    return getattr(F, name), (op, series, weight, bias, bias_kind, mode), (series, weight, bias)


def run(spec):
    """one row's result: {"error", "calls"} of a refused call, {"shape", "calls", "nulls"} of an accepted one"""
    spec = dict(DEFAULTS, **spec)
    with pytest.MonkeyPatch.context() as mp:
        rec = _TableRecorder(spec["plan"] == "refuses")
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
        if spec["auto"] == "all":
            mp.setattr(F, "SERIES_FUSED_AUTO", ("windows_f1", "series"))
            mp.setattr(F, "SERIES_POOL_FUSED_AUTO", ("pool", "pool_dropout"))
        fn, args, leaves = _arguments(spec)
        train = spec["train"] != "no"
        if train:
            for i, t in enumerate(leaves):
                t.requires_grad_(not (i == 1 and spec["train"] == "frozen"))
        kw = dict(ENTRIES[spec["entry"]][2], **GEOMETRIES[spec["geom"]])
        kw.update(spec["kw"], as_series=spec["as_series"])
        try:
            with (torch.enable_grad() if train else torch.no_grad()):
                z = fn(*args, **kw)
                if train:
                    z.backward(torch.ones_like(z))
        except _lib.TgcnError as e:
            return {"error": str(e), "calls": list(rec.calls)}
        return {"shape": list(z.shape), "calls": list(rec.calls), "nulls": [list(n) for n in rec.nulls]}


def table():
    """{"rows": {key: index into results}, "results": [...]}: rows in the grid's order, equal results stored once"""
    rows, results, index = {}, [], {}
    for spec in grid():
        text = json.dumps(run(spec), sort_keys=True)
        if text not in index:
            index[text] = len(results)
            results.append(json.loads(text))
        rows[key_of(spec)] = index[text]
    return {"rows": rows, "results": results}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_row_does_what_the_recording_did(recorded):
    specs = grid()
    assert [key_of(s) for s in specs] == list(recorded["rows"])
    wrong = []
    for spec in specs:
        now, then = run(spec), recorded["results"][recorded["rows"][key_of(spec)]]
        if now != then:
            wrong.append((key_of(spec), now, then))
    assert not wrong, "%d rows differ; (row, now, recorded) of the first: %s" % (len(wrong), wrong[:3])


# a fragment of every refusal the five functions and the four wrappers document
REFUSALS = [
    "bfloat16 parameters are not supported", "a (S, n, T) series takes a (K, H, N) weight", "channels, the weight", "pool is 2 or 4",
    "are not a multiple of pool", "padding is an int, a pair", "outside 0 ..", "stride is an integer >= 1", "dilation is an integer >= 1",
    "together with stride", "are fewer than one window", "p is a real number in [0, 1)", "seed is None, an integer", "a seed tensor is one int64",
    "time_chunk is None or an integer >= 1, got 0", "got None -- without chunks", 'padding="causal" only', "time_chunk runs at stride=1 only",
    "time_chunk runs in float32 only", "fused is True or \"auto\"", "fused is False, True or \"auto\"", "fused=True runs in float32 only",
    "fused=True has no window step", "fused=True does not walk time chunks", "fused=True needs a square operand",
    "a reordered operand is not supported", "do not fit the one-launch layer", "learnable edge weights", "the layer is a TGCNCheb_H or a ChebTimeConv",
    "after the series", "the series is (S, n, T) or (S, n, T, f)", "channel(s), the layer in_channels", "the scalar-load form",
    "the parameters are bfloat16 but the series is",
]


def test_the_recording_is_small_and_covers_the_family(recorded):
    rows, results = recorded["rows"], recorded["results"]
    assert len(rows) <= 1000 and os.path.getsize(GOLDEN) < 256 * 1024
    assert sorted(set(rows.values())) == list(range(len(results)))
    accepted = sum("shape" in results[i] for i in rows.values())
    assert accepted >= 0.4 * len(rows), (accepted, len(rows))
    errors = {(key.split()[0], results[i]["error"]) for key, i in rows.items() if "error" in results[i]}
    for entry in ENTRIES:
        assert any("shape" in results[i] and results[i]["calls"] for key, i in rows.items() if key.split()[0] == entry), entry
        assert sum(e == entry for e, _ in errors) >= 10, entry
    for text in REFUSALS:
        assert any(text in msg for _, msg in errors), text
