#!/usr/bin/env python3
"""forward_series on multi-channel series against the only thing the modules offered for those shapes before: the same module's forward on
the materialised windowed batch xw[s*nwin + w, i, h, c] = series[s, i, w + h, c] (built once, outside the timed region).  Events around the
call, ms per call and per kernel kind (tgcn_profile_*), forward and forward + backward.  Developer tool; bench.py's headline is untouched.

    python tools/series_bench.py [--steps 5] [--warmup 2] [--stride 1] [--padding 0] [--conv] [--out profiles/r08_series_channels.json]
    python tools/series_bench.py --dtype bf16 [--out profiles/r10_series_bf16.json]
    python tools/series_bench.py --dilation [--out profiles/r11_series_dilation.json]
    python tools/series_bench.py --stream [--out profiles/r12_series_stream.json]
    python tools/series_bench.py --stream --graph [--include parent=FILE] [--out profiles/r13_series_stream_graph.json]
    python tools/series_bench.py --stream --fused [--include parent=FILE] [--out profiles/r14_series_stream_fused.json]
    python tools/series_bench.py --stream --stride 2,2,2 [--repeats 3] [--include parent=FILE] [--out profiles/r16_series_stream_stride.json]
    python tools/series_bench.py --time-chunk 64,256 [--repeats 3] [--include parent=FILE] [--out profiles/r17_series_time_chunk.json]
    python tools/series_bench.py --fused-series --steps 200 --warmup 20 [--repeats 3] [--include parent=FILE] [--out profiles/r21_series_small.json]
    python tools/series_bench.py --fused-series --relu-pool 4 [--dropout 0.5] --steps 200 --warmup 20 [--include LABEL=FILE] [--out profiles/r24_series_small_pool.json]
    python tools/series_bench.py --relu-pool 4 [--repeats 3] [--out profiles/r18_series_relu_pool.json]
    python tools/series_bench.py --relu-pool 4 --dropout 0.1 [--repeats 3] [--out profiles/r22_series_relu_dropout_pool.json]
    python tools/series_bench.py --time-chunk 32,64 --relu-pool 4 [--dropout 0.1] [--repeats 3] [--out profiles/r23_series_chunk_relu_pool.json]

Cases: (a) the 148-parcel DTI graph, S = 8 recordings of T = 284, H = 15, K = 10, the two layers of the reference's HCP net (1 -> 32 and
32 -> 64 channels); (b) the 90 k-vertex sheet mesh, S = 1, T = 75, H = 15, 4 -> 32 channels, K = 5; (c) the two layers of (a) chained:
streaming passes the first layer's output on as a series (as_series=True), the baseline cuts the second layer's windows out of the first
layer's output inside the timed region (it has to: they do not exist before).
--stride / --padding (an int, "left,right" or "causal") run (a) and (b) with that geometry (the baseline's windows are cut with it too, outside
the timed region); --conv adds the cases of profiles/r09_series_conv.json: (a) 32 -> 64 and (b) at stride 4, and chain (c) with
padding="causal" in both layers (284 time steps in, 284 out).  --include LABEL=FILE (repeatable) embeds the --out file of another run --
the parent commit's tool on the default cases, a repeat of this one for the run-to-run spread -- with its times relative to this run's.
--dtype bf16 runs cases (a) 32 -> 64, (b) and (c) with bfloat16 layers (forward_series on bf16 tensors, DESIGN.md 3.10 "bf16") and, on the same
commit, the fp32 streaming call and the bf16 module's forward on the materialised windows; default --out profiles/r10_series_bf16.json.
--dilation runs the dilated cases (DESIGN.md 3.10 "Dilation"): (a) 32 -> 64 and (b) at dilation 4, and a three-layer causal chain of H = 5
layers with dilations 1, 2, 4 (1 -> 32 -> 32 -> 64 channels, 284 steps in, 284 out, receptive field 29 steps), each next to the module's forward on
the materialised dilated windows on the same commit; default --out profiles/r11_series_dilation.json.
--stream times the streaming state (DESIGN.md 3.10 "Streaming state"): ms per chunk of that three-layer causal chain through forward_stream at
chunk sizes 1, 8 and 64 (states warmed by 64 time rows), next to what a caller has to do without it on the same commit -- keep the trailing
He - 1 + Tc input rows of every layer and run forward_series on them; default --out profiles/r12_series_stream.json.
--stream --graph times that chain's step captured into one hipGraph (tgcn_amd.GraphedStream, states with capturable=True) next to the eager
forward_stream step on the same commit, at chunk sizes 1, 8 and 64, and records whether the two gave torch.equal outputs over the warm-up
recording; --include LABEL=FILE embeds a --stream run of another commit (the parent's eager column); default --out
profiles/r13_series_stream_graph.json.
--stream --fused times that chain's step in one launch per layer (forward_stream(..., fused=True), DESIGN.md 3.10 "One launch per step")
next to the eager host-head step (fused=False, the code the parent commit runs) and the GraphedStream replay of the fused step, at chunk
sizes 1, 8 and 64: three repeats of each, events only (no launch record inside a timed region), the library launches of one step of each
counted in a separate untimed step, and the largest relative difference of fused and eager outputs over the warm-up recording.  --include
LABEL=FILE embeds a --stream --graph run of the parent commit (its eager_ms_per_chunk is the comparison column); default --out
profiles/r14_series_stream_fused.json.
--stream --stride S1,S2,S3 times that three-layer chain undilated with the window steps S1, S2, S3 (forward_stream(..., stride=s), DESIGN.md
3.10 "Window step") at chunks of S1*S2*S3, 64 and 512 time rows, next to what a caller does without the keyword: the same chain through the
step-1 forward_stream with every layer's output sliced out[:, :, ::s] before the next layer.  Per column: --repeats event timings of --steps
chunks each (ms per chunk, their median and spread) and one pass with the launch record.  On a tree whose forward_stream has no `stride`
keyword only the sliced column is timed, which is how the parent commit's file for --include LABEL=FILE is made; default --out
profiles/r16_series_stream_stride.json.
--time-chunk Tc[,Tc...] times a training step (forward + backward, all three gradients) of forward_series(..., padding="causal") on long
recordings, T = 1200: (a) 32 -> 64 and (b), the unchunked call against time_chunk=Tc for each Tc (DESIGN.md 3.10 "Time chunks"), in the same
run, alternating, --repeats event timings of --steps steps each, and torch.cuda.max_memory_allocated above the allocation before the step.
On a tree whose forward_series has no `time_chunk` keyword only the unchunked column is taken, which is how the parent commit's file for
--include LABEL=FILE is made; default --out profiles/r17_series_time_chunk.json.
--relu-pool P (2 or 4) times tgcn_amd.cheb_series_relu_pool(layer, series, pool=P) against the hand-written composition
gcn_pool_4(relu(layer.forward_series(series))) (P = 2: gcn_pool; on the series layout through the (S, n, nwin*g) view) on the same commit:
case (a) at 1 -> 32 window-major and at 32 -> 64 in the series layout, and case (b), forward and forward + backward.  The two sides
alternate within the run, --repeats event timings each (median and spread); per side the peak of max_memory_allocated above the pre-call
level, and torch.equal of the results and of every gradient; default --out profiles/r18_series_relu_pool.json.
--relu-pool P --dropout PROB (0 < PROB < 1) puts dropout between relu and the pool on the same cases: (a) the fused call
tgcn_amd.cheb_series_relu_dropout_pool(layer, series, p=PROB, pool=P) with seed=None, (b) the composition forward_series -> relu ->
torch's F.dropout -> gcn_pool_4 and (c) cheb_series_relu_pool without dropout -- the column to hold against a --relu-pool P run of the
parent commit, whose code it shares.  The three alternate within the run; medians, spreads and peaks as above.  The masks of (a) and (b)
are different generators', so no equality is recorded; default --out profiles/r22_series_relu_dropout_pool.json.
--time-chunk Tc[,Tc...] --relu-pool P [--dropout PROB] times a training step (forward + backward, all three gradients) of the causal layer
followed by relu (+ dropout) + pool on the three cases of --relu-pool (DESIGN.md 3.10 "Time chunks through the pooled epilogue"), three forms
in one run, alternating: (a) the fused unchunked call, cheb_series_relu_pool / cheb_series_relu_dropout_pool(..., padding="causal"); and
per Tc (b) forward_series(..., padding="causal", time_chunk=Tc) followed by the stand-alone relu (+ dropout) + pool pass and (c)
cheb_series_relu_pool_chunked(..., time_chunk=Tc).  One seed for the three, so they compute the same z.  Per column --repeats event
timings of --steps steps each (median and spread) and the peak of max_memory_allocated above the pre-step level, also in units of the
layer's full output; default --out profiles/r23_series_chunk_relu_pool.json.
--fused-series: the one-launch whole-series layer (forward_series(fused=True), DESIGN.md 3.10 "One launch per series") on the graphs that fit
in LDS: the (a) layers of the r08 table on the 148 parcels (1 -> 32 window-major and as_series=True; 32 -> 64, which the plan refuses) and
TGCNCheb_H(L, 1, 64, 5, 28) on the 28 x 28 grid, S = 8, T = 128.  Columns per case, forward and forward + backward: unfused and fused
forward_series and forward on the materialised windows, alternating within the run, --repeats event timings of --steps calls each (median
and max - min).  On a commit without the keyword only the unfused and the materialised column are timed, which is how the parent commit's file
for --include LABEL=FILE is made; default --out profiles/r21_series_small.json.
--fused-series --relu-pool P [--dropout PROB]: relu (+ dropout) + pool behind the one-launch layer (DESIGN.md 3.10 "relu + pool in the one-launch
series layer") on the two fusable operands of r21 (148 parcels 1 -> 32, the 28 x 28 grid), window-major, forward and forward + backward:
(a) tgcn_amd.cheb_series_relu_pool_fused, (b) cheb_series_relu_pool / cheb_series_relu_dropout_pool, the general pooled epilogue, and (c)
forward_series(fused=True) followed by the relu (+ dropout) + pool pass -- alternating, --repeats event timings of --steps calls each.  One
row per (case, direction) with its class ("pool" / "pool_dropout"); on a commit without (a) only (b) and (c) are timed, which is how the
parent's file is made.  --include LABEL=FILE appends another run's rows under that label -- the parent's build, or this tool's run with the
other --dropout setting under the label "this", so that one file holds both classes -- and "auto" is F.SERIES_POOL_FUSED_AUTO's rule over
the rows labelled "this"; default --out profiles/r24_series_small_pool.json."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tgcn_amd  # noqa: E402
from tgcn_amd import _lib  # noqa: E402
from tgcn_amd import functional as F  # noqa: E402
from tgcn_amd.graph import GraphOperand  # noqa: E402
from tools import synth  # noqa: E402
from tools.precision_bench import measure  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def dti148(dev):
    z = np.load(os.path.join(GOLDEN, "TGCNChebH_dti148_q4_f1_g32_K10_H15.npz"))
    n = int(z["n"])
    rowptr = torch.as_tensor(z["rowptr"]).long()
    row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    return GraphOperand.from_coo(n, row.to(dev), torch.as_tensor(z["col"]).long().to(dev), torch.as_tensor(z["val"]).float().to(dev))


def windows(series, H, stride=1, padding=0):
    """(S, n, T, f) -> (S*nwin, n, H, f), contiguous: every stride-th window of the zero-padded series"""
    S, n, T, f = series.shape
    left, right = F.series_geometry(T, H, stride, padding)[1:3]
    if left or right:
        series = torch.nn.functional.pad(series, (0, 0, left, right))
    w = series.unfold(2, H, stride)                                        # (S, n, nwin, f, H)
    return w.permute(0, 2, 1, 4, 3).reshape(S * w.shape[2], n, H, f).contiguous()


def windows_dilated(series, H, dilation, padding=0):
    """(S, n, T, f) -> (S*nwin, n, H, f), contiguous: the windows of the zero-padded series whose taps lie `dilation` time rows apart"""
    S, n, T, f = series.shape
    left, right, nwin = F.series_geometry(T, H, 1, padding, dilation=dilation)[1:]
    if left or right:
        series = torch.nn.functional.pad(series, (0, 0, left, right))
    idx = torch.arange(nwin, device=series.device)[:, None] + torch.arange(H, device=series.device)[None, :] * dilation
    return series[:, :, idx].permute(0, 2, 1, 3, 4).reshape(S * nwin, n, H, f).contiguous()


def padding_arg(text):
    if text == "causal":
        return text
    parts = [int(v) for v in text.split(",")]
    return parts[0] if len(parts) == 1 else tuple(parts)


def timed(fn, train, steps, warmup):
    def call():
        if train:
            out = fn()
            out.backward(torch.ones_like(out))
        else:
            with torch.no_grad():
                fn()
    r, _ = measure(call, steps, warmup)
    if train:
        r["note"] = "kernel times cover the forward only: the backward runs on autograd's thread, which the thread-local launch record does not see"
    return r


def compare(stream, batch, steps, warmup):
    out = {}
    for train in (False, True):
        s, b = timed(stream, train, steps, warmup), timed(batch, train, steps, warmup)
        out["forward_backward" if train else "forward"] = dict(streaming=s, materialised=b,
                                                                materialised_over_streaming=round(b["ms_per_call"] / s["ms_per_call"], 3))
    return out


def compare_bf16(stream_bf16, stream_fp32, batch_bf16, steps, warmup):
    out = {}
    for train in (False, True):
        s, f32, b = (timed(fn, train, steps, warmup) for fn in (stream_bf16, stream_fp32, batch_bf16))
        out["forward_backward" if train else "forward"] = dict(streaming_bf16=s, streaming_fp32=f32, materialised_bf16=b,
                                                                fp32_over_bf16=round(f32["ms_per_call"] / s["ms_per_call"], 3),
                                                                materialised_over_streaming=round(b["ms_per_call"] / s["ms_per_call"], 3))
    return out


def main_bf16(args):
    import copy
    BF = torch.bfloat16
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, dtype="bf16", cases={})
    torch.manual_seed(0)

    def record(name, entry):
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        torch.cuda.empty_cache()

    def case(name, desc, layer, series, H):
        lb = copy.deepcopy(layer).to(BF)
        s32, sb = series.requires_grad_(True), series.detach().to(BF).requires_grad_(True)
        xw = windows(series.detach(), H).to(BF).requires_grad_(True)
        record(name, dict(desc=desc, **compare_bf16(lambda: lb.forward_series(sb), lambda: layer.forward_series(s32), lambda: lb(xw),
                                                    args.steps, args.warmup)))

    op = dti148(dev)
    S, T, H, K = 8, 284, 15, 10
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 32, K, H).to(dev)
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, K, H).to(dev)
    case("a_dti148_32to64", "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64", l2, torch.randn(S, op.n, T, 32, device=dev), H)
    n, row, col, val = synth.sheet_mesh(300, device=dev)
    opm = GraphOperand.from_coo(n, row, col, val, dev)
    lm = tgcn_amd.TGCNCheb_H(opm, 4, 32, 5, 15).to(dev)
    case("b_mesh90k_4to32", "sheet_mesh(300) n=%d S=1 T=75 H=15 K=5 f=4 -> g=32" % n, lm, torch.randn(1, n, 75, 4, device=dev), 15)
    del lm, opm
    torch.cuda.empty_cache()

    l1b, l2b = copy.deepcopy(l1).to(BF), copy.deepcopy(l2).to(BF)
    series = torch.randn(S, op.n, T, 1, device=dev).requires_grad_(True)
    sb = series.detach().to(BF).requires_grad_(True)
    xw1 = windows(series.detach(), H).to(BF).requires_grad_(True)
    T1 = T - H + 1

    def chain_batch():
        h = torch.relu(l1b(xw1))                                          # (S*T1, n, 32)
        return l2b(windows(h.view(S, T1, op.n, 32).permute(0, 2, 1, 3), H))
    record("c_dti148_chain", dict(desc="dti148 S=8 T=284: TGCNCheb_H(1,32,10,15) -> relu -> TGCNCheb_H(32,64,10,15)",
                                  **compare_bf16(lambda: l2b.forward_series(torch.relu(l1b.forward_series(sb, as_series=True))),
                                                 lambda: l2.forward_series(torch.relu(l1.forward_series(series, as_series=True))),
                                                 chain_batch, args.steps, args.warmup)))
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r10_series_bf16.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_dilation(args):
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, cases={})
    torch.manual_seed(0)

    def record(name, entry):
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        torch.cuda.empty_cache()

    def case(name, desc, layer, series, H, d):
        series = series.requires_grad_(True)
        xw = windows_dilated(series.detach(), H, d).requires_grad_(True)
        record(name, dict(desc=desc + " dilation=%d" % d, **compare(lambda: layer.forward_series(series, dilation=d), lambda: layer(xw),
                                                                   args.steps, args.warmup)))

    op = dti148(dev)
    S, T, H, K = 8, 284, 15, 10
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, K, H).to(dev)
    case("a_dti148_32to64_dilation4", "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64", l2, torch.randn(S, op.n, T, 32, device=dev), H, 4)
    del l2
    n, row, col, val = synth.sheet_mesh(300, device=dev)
    opm = GraphOperand.from_coo(n, row, col, val, dev)
    lm = tgcn_amd.TGCNCheb_H(opm, 4, 32, 5, 15).to(dev)
    case("b_mesh90k_4to32_dilation4", "sheet_mesh(300) n=%d S=1 T=75 H=15 K=5 f=4 -> g=32" % n, lm, torch.randn(1, n, 75, 4, device=dev), 15, 4)
    del lm, opm
    torch.cuda.empty_cache()

    Hc, dils, chans = 5, (1, 2, 4), (1, 32, 32, 64)
    layers = [tgcn_amd.TGCNCheb_H(op, chans[i], chans[i + 1], K, Hc).to(dev) for i in range(3)]
    series = torch.randn(S, op.n, T, 1, device=dev).requires_grad_(True)

    def chain_stream():
        h = series
        for i, (layer, d) in enumerate(zip(layers, dils)):
            h = layer.forward_series(h, as_series=True, padding="causal", dilation=d)
            if i < 2:
                h = torch.relu(h)
        return h

    def chain_batch():          # every layer's windows are cut from the previous layer's output inside the timed region: they do not exist before
        h = series
        for i, (layer, d) in enumerate(zip(layers, dils)):
            y = layer(windows_dilated(h, Hc, d, "causal"))               # (S*T, n, g)
            h = y.view(S, T, op.n, -1).permute(0, 2, 1, 3)
            if i < 2:
                h = torch.relu(h)
        return h
    record("c_dti148_chain_dilated", dict(desc="dti148 S=8 T=284: three causal TGCNCheb_H(., ., 10, 5) layers 1 -> 32 -> 32 -> 64 with dilations 1, 2, 4",
                                          **compare(chain_stream, chain_batch, args.steps, args.warmup)))
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r11_series_dilation.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_stream(args):
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, cases={})
    torch.manual_seed(0)
    op = dti148(dev)
    S, K, Hc, dils, chans = 8, 10, 5, (1, 2, 4), (1, 32, 32, 64)
    layers = [tgcn_amd.TGCNCheb_H(op, chans[i], chans[i + 1], K, Hc).to(dev) for i in range(3)]
    for Tc in (1, 8, 64):
        chunk = torch.randn(S, op.n, Tc, 1, device=dev)
        states = [None] * 3

        def stream_step(x=chunk):
            h = x
            for i, (layer, d) in enumerate(zip(layers, dils)):
                h, states[i] = layer.forward_stream(h, states[i], dilation=d)
                if i < 2:
                    h = torch.relu(h)
            return h

        # without the state: every layer's caller keeps the last He - 1 + Tc rows of that layer's input and runs forward_series on them
        tails = [torch.zeros(S, op.n, (Hc - 1) * d + Tc, chans[i], device=dev) for i, d in enumerate(dils)]

        def trailing_step(x=chunk):
            h = x
            for i, (layer, d) in enumerate(zip(layers, dils)):
                tails[i] = torch.cat((tails[i][:, :, h.shape[2]:], h), dim=2)
                h = layer.forward_series(tails[i], as_series=True, dilation=d)          # the Tc newest outputs
                if i < 2:
                    h = torch.relu(h)
            return h

        with torch.no_grad():
            for _ in range(-(-64 // Tc)):
                a, b = stream_step(), trailing_step()
            assert a.shape == b.shape == (S, op.n, Tc, chans[-1])
            err = float((a - b).abs().max() / b.abs().max())
        st, tr = timed(stream_step, False, args.steps, args.warmup), timed(trailing_step, False, args.steps, args.warmup)
        entry = dict(desc="dti148 S=8: three causal TGCNCheb_H(., ., 10, 5) layers 1 -> 32 -> 32 -> 64 with dilations 1, 2, 4, chunks of %d time rows" % Tc,
                     forward_stream=st, forward_series_on_trailing_rows=tr, max_rel_difference=err,
                     trailing_over_stream=round(tr["ms_per_call"] / st["ms_per_call"], 3))
        res["cases"]["chain_chunk%d" % Tc] = entry
        print(json.dumps({"chain_chunk%d" % Tc: entry}), flush=True)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r12_series_stream.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def events_ms(fn, steps, warmup):
    """ms per call between two events, no launch record: the record's own events would be host work inside a step that is host-bound"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / steps, 4)


def main_stream_graph(args):
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, cases={})
    torch.manual_seed(0)
    op = dti148(dev)
    S, K, Hc, dils, chans = 8, 10, 5, (1, 2, 4), (1, 32, 32, 64)
    layers = [tgcn_amd.TGCNCheb_H(op, chans[i], chans[i + 1], K, Hc).to(dev) for i in range(3)]

    def chain(capturable):
        def step(x, states):
            states = list(states or [None] * 3)
            h = x
            for i, (layer, d) in enumerate(zip(layers, dils)):
                h, states[i] = layer.forward_stream(h, state=states[i], dilation=d, capturable=capturable)
                if i < 2:
                    h = torch.relu(h)
            return h, states
        return step

    for Tc in (1, 8, 64):
        chunk = torch.randn(S, op.n, Tc, 1, device=dev)
        eager, host = chain(False), [None]
        gs = tgcn_amd.GraphedStream(chain(True), chunk)

        def eager_step(x=chunk):
            out, host[0] = eager(x, host[0])
            return out

        def graph_step(x=chunk):
            return gs(x)

        equal = True
        with torch.no_grad():
            for _ in range(-(-64 // Tc)):           # one recording of 64 time rows through both, chunk by chunk
                x = torch.randn(S, op.n, Tc, 1, device=dev)
                equal = equal and bool(torch.equal(eager_step(x), graph_step(x)))
            recorded = timed(eager_step, False, args.steps, args.warmup)        # with the launch record, as --stream times it
            e_ms = events_ms(eager_step, args.steps, args.warmup)
        g_ms = events_ms(graph_step, args.steps, args.warmup)
        entry = dict(desc="dti148 S=8: three causal TGCNCheb_H(., ., 10, 5) layers 1 -> 32 -> 32 -> 64 with dilations 1, 2, 4, chunks of %d time rows" % Tc,
                     forward_stream=recorded, eager_ms_per_chunk=e_ms, graphed_ms_per_chunk=g_ms, outputs_torch_equal=equal,
                     eager_over_graphed=round(e_ms / g_ms, 3))
        res["cases"]["chain_chunk%d" % Tc] = entry
        print(json.dumps({"chain_chunk%d" % Tc: entry}), flush=True)
        del gs
    for item in args.include:
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        rel = {name: round(entry["forward_stream"]["ms_per_call"] / res["cases"][name]["forward_stream"]["ms_per_call"], 3)
               for name, entry in other["cases"].items() if name in res["cases"]}
        res.setdefault("runs", {})[label] = dict(run=other, forward_stream_ms_over_this_run=rel)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r13_series_stream_graph.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def launches_of(fn):
    """library launches of one call, by kind (the launch record, outside every timed region)"""
    torch.cuda.synchronize()
    _lib.profile_start(1 << 12)
    with torch.no_grad():
        fn()
    torch.cuda.synchronize()
    kinds = [k for k, _ in _lib.profile_stop(1 << 12)]
    return len(kinds)


def main_stream_fused(args):
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=3,
               auto_max_tc=F.STREAM_FUSED_AUTO_MAX_TC, cases={})
    torch.manual_seed(0)
    op = dti148(dev)
    S, K, Hc, dils, chans = 8, 10, 5, (1, 2, 4), (1, 32, 32, 64)
    layers = [tgcn_amd.TGCNCheb_H(op, chans[i], chans[i + 1], K, Hc).to(dev) for i in range(3)]

    def chain(capturable, fused):
        def step(x, states):
            states = list(states or [None] * 3)
            h = x
            for i, (layer, d) in enumerate(zip(layers, dils)):
                h, states[i] = layer.forward_stream(h, state=states[i], dilation=d, capturable=capturable, fused=fused)
                if i < 2:
                    h = torch.relu(h)
            return h, states
        return step

    for Tc in (1, 8, 64):
        chunk = torch.randn(S, op.n, Tc, 1, device=dev)
        plans = [F._stream_small_plan(op, chans[i], Hc, chans[i + 1], K, Tc, dils[i], F.MODE_POWER) for i in range(3)]
        eager, fused, cap = chain(False, False), chain(False, True), chain(True, True)
        st_e, st_f, st_c = [None], [None], [None]
        gs = tgcn_amd.GraphedStream(cap, chunk)

        def eager_step(x=chunk):
            out, st_e[0] = eager(x, st_e[0])
            return out

        def fused_step(x=chunk):
            out, st_f[0] = fused(x, st_f[0])
            return out

        def cap_step(x=chunk):
            out, st_c[0] = cap(x, st_c[0])
            return out

        def graph_step(x=chunk):
            return gs(x)

        err, equal = 0.0, True
        with torch.no_grad():
            for _ in range(-(-64 // Tc)):           # one recording of 64 time rows through all three, chunk by chunk
                x = torch.randn(S, op.n, Tc, 1, device=dev)
                a, b, c = eager_step(x), fused_step(x), graph_step(x)
                err = max(err, float((a - b).abs().max() / a.abs().max()))
                equal = equal and bool(torch.equal(b, c))
            counts = dict(eager=launches_of(eager_step), fused=launches_of(fused_step), graphed_fused=launches_of(cap_step))
            e_ms = [events_ms(eager_step, args.steps, args.warmup) for _ in range(3)]
            f_ms = [events_ms(fused_step, args.steps, args.warmup) for _ in range(3)]
        g_ms = [events_ms(graph_step, args.steps, args.warmup) for _ in range(3)]
        med = lambda v: sorted(v)[1]      # noqa: E731
        entry = dict(desc="dti148 S=8: three causal TGCNCheb_H(., ., 10, 5) layers 1 -> 32 -> 32 -> 64 with dilations 1, 2, 4, chunks of %d time rows" % Tc,
                     plans=[dict(rc=rc, tb=tb, dense=dn, lds_bytes=lds) for rc, tb, dn, lds in plans],
                     eager_ms_per_chunk=e_ms, fused_ms_per_chunk=f_ms, graphed_fused_ms_per_chunk=g_ms,
                     spread_ms=dict(eager=round(max(e_ms) - min(e_ms), 4), fused=round(max(f_ms) - min(f_ms), 4),
                                    graphed_fused=round(max(g_ms) - min(g_ms), 4)),
                     library_launches_per_chunk=counts, max_rel_difference_fused_vs_eager=err, graphed_fused_torch_equal_fused=equal,
                     eager_over_fused=round(med(e_ms) / med(f_ms), 3), eager_over_graphed_fused=round(med(e_ms) / med(g_ms), 3))
        res["cases"]["chain_chunk%d" % Tc] = entry
        print(json.dumps({"chain_chunk%d" % Tc: entry}), flush=True)
        del gs
    for item in args.include:
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        rel = {name: round(entry["eager_ms_per_chunk"] / sorted(res["cases"][name]["eager_ms_per_chunk"])[1], 3)
               for name, entry in other["cases"].items() if name in res["cases"]}
        res.setdefault("runs", {})[label] = dict(run=other, eager_ms_over_this_run=rel)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r14_series_stream_fused.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_stream_stride(args):
    import inspect
    dev = torch.device("cuda:0")
    steps3 = args.stride
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               strides=list(steps3), cases={})
    torch.manual_seed(0)
    op = dti148(dev)
    S, K, Hc, chans = 8, 10, 5, (1, 32, 32, 64)
    layers = [tgcn_amd.TGCNCheb_H(op, chans[i], chans[i + 1], K, Hc).to(dev) for i in range(3)]
    has_step = "stride" in inspect.signature(tgcn_amd.TGCNCheb_H.forward_stream).parameters
    whole = steps3[0] * steps3[1] * steps3[2]

    def repeated(fn):
        ms = [events_ms(fn, args.steps, args.warmup) for _ in range(args.repeats)]
        return dict(ms_per_chunk=ms, median=sorted(ms)[len(ms) // 2], spread=round(max(ms) - min(ms), 4))

    for Tc in sorted({whole, -(-64 // whole) * whole, -(-512 // whole) * whole}):        # chunks of whole steps: the sliced chain's phase is 0 on every chunk
        chunk = torch.randn(S, op.n, Tc, 1, device=dev)
        st_states, sl_states = [None] * 3, [None] * 3

        def strided_step(x=chunk):
            h = x
            for i, (layer, s) in enumerate(zip(layers, steps3)):
                h, st_states[i] = layer.forward_stream(h, st_states[i], stride=s)
                if i < 2:
                    h = torch.relu(h)
            return h

        # without the keyword: every layer at step 1, every window projected, s - 1 of s of them dropped by the caller
        def sliced_step(x=chunk):
            h = x
            for i, (layer, s) in enumerate(zip(layers, steps3)):
                h, sl_states[i] = layer.forward_stream(h, sl_states[i])
                h = h[:, :, ::s].contiguous()
                if i < 2:
                    h = torch.relu(h)
            return h

        entry = dict(desc="dti148 S=8: three causal TGCNCheb_H(., ., 10, 5) layers 1 -> 32 -> 32 -> 64 with window steps %d, %d, %d, chunks of %d "
                          "time rows" % (steps3 + (Tc,)))
        with torch.no_grad():
            for _ in range(-(-64 // Tc)):
                b = sliced_step()
                if has_step:
                    a = strided_step()
                    assert a.shape == b.shape == (S, op.n, Tc // whole, chans[-1])
                    entry["max_rel_difference"] = float((a - b).abs().max() / b.abs().max())
            entry["step1_sliced"] = dict(repeated(sliced_step), record=timed(sliced_step, False, args.steps, args.warmup))
            if has_step:
                entry["strided"] = dict(repeated(strided_step), record=timed(strided_step, False, args.steps, args.warmup))
                entry["sliced_over_strided"] = round(entry["step1_sliced"]["median"] / entry["strided"]["median"], 3)
        res["cases"]["chain_chunk%d" % Tc] = entry
        print(json.dumps({"chain_chunk%d" % Tc: entry}), flush=True)
    for item in args.include:
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        rel = {name: round(entry["step1_sliced"]["median"] / res["cases"][name]["step1_sliced"]["median"], 3)
               for name, entry in other["cases"].items() if name in res["cases"]}
        res.setdefault("runs", {})[label] = dict(run=other, step1_sliced_ms_over_this_run=rel)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r16_series_stream_stride.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_time_chunk(args):
    import inspect
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               time_chunks=list(args.time_chunk), T=1200, cases={})
    torch.manual_seed(0)
    has_kw = "time_chunk" in inspect.signature(tgcn_amd.TGCNCheb_H.forward_series).parameters
    columns = [None] + (list(args.time_chunk) if has_kw else [])
    T = 1200

    def case(name, desc, layer, series):
        series = series.requires_grad_(True)

        def step_of(tc):
            kw = {} if tc is None else dict(time_chunk=tc)

            def step():
                layer.zero_grad(set_to_none=True)
                series.grad = None
                out = layer.forward_series(series, as_series=True, padding="causal", **kw)
                out.backward(torch.ones_like(out))
            return step

        ms, peak = {c: [] for c in columns}, {}
        for _ in range(args.repeats):               # alternating: every column once per repeat
            for c in columns:
                step = step_of(c)
                ms[c].append(events_ms(step, args.steps, args.warmup))
                layer.zero_grad(set_to_none=True)
                series.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                peak[c] = torch.cuda.max_memory_allocated() - base
        label = lambda c: "unchunked" if c is None else "time_chunk_%d" % c      # noqa: E731
        entry = dict(desc=desc, series_bytes=series.numel() * 4)
        for c in columns:
            entry[label(c)] = dict(ms_per_step=ms[c], median=sorted(ms[c])[len(ms[c]) // 2], spread=round(max(ms[c]) - min(ms[c]), 4),
                                   peak_bytes_above_baseline=peak[c], peak_over_series_bytes=round(peak[c] / (series.numel() * 4), 2))
            if c is not None:
                entry[label(c)]["ms_over_unchunked"] = round(entry[label(c)]["median"] / entry["unchunked"]["median"], 3)
                entry[label(c)]["peak_over_unchunked"] = round(peak[c] / peak[None], 3)
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        layer.zero_grad(set_to_none=True)
        series.grad = None
        torch.cuda.empty_cache()

    op = dti148(dev)
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, 10, 15).to(dev)
    case("a_dti148_32to64_T1200", "dti148 S=8 T=1200 H=15 K=10 f=32 -> g=64 causal, forward + backward", l2, torch.randn(8, op.n, T, 32, device=dev))
    del l2
    n, row, col, val = synth.sheet_mesh(300, device=dev)
    opm = GraphOperand.from_coo(n, row, col, val, dev)
    lm = tgcn_amd.TGCNCheb_H(opm, 4, 32, 5, 15).to(dev)
    case("b_mesh90k_4to32_T1200", "sheet_mesh(300) n=%d S=1 T=1200 H=15 K=5 f=4 -> g=32 causal, forward + backward" % n, lm,
         torch.randn(1, n, T, 4, device=dev))
    for item in args.include:
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        rel = {name: round(entry["unchunked"]["median"] / res["cases"][name]["unchunked"]["median"], 3)
               for name, entry in other["cases"].items() if name in res["cases"]}
        res.setdefault("runs", {})[label] = dict(run=other, unchunked_ms_over_this_run=rel)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r17_series_time_chunk.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_relu_pool(args):
    dev = torch.device("cuda:0")
    pool = args.relu_pool
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               pool=pool, cases={})
    drop = args.dropout
    if drop is not None:
        res["dropout"] = drop
    torch.manual_seed(0)
    pool_fn = tgcn_amd.gcn_pool_4 if pool == 4 else tgcn_amd.gcn_pool

    def case(name, desc, layer, series, as_series):
        series = series.requires_grad_(True)

        def undropped():
            return tgcn_amd.cheb_series_relu_pool(layer, series, pool=pool, as_series=as_series)

        def fused():
            if drop is None:
                return undropped()
            return tgcn_amd.cheb_series_relu_dropout_pool(layer, series, p=drop, pool=pool, as_series=as_series)

        def composition():
            out = torch.relu(layer.forward_series(series, as_series=as_series))
            if drop is not None:
                out = torch.nn.functional.dropout(out, drop, True)
            if not as_series:
                return pool_fn(out)
            S, n, nwin, g = out.shape
            return pool_fn(out.view(S, n, -1)).view(S, n // pool, nwin, g)

        def clear():
            layer.zero_grad(set_to_none=True)
            series.grad = None

        def step_of(fn, train):
            def step():
                if train:
                    clear()
                    z = fn()
                    z.backward(torch.ones_like(z))
                else:
                    with torch.no_grad():
                        fn()
            return step

        sides = (("fused", fused), ("composition", composition)) + ((("undropped", undropped),) if drop is not None else ())
        entry = dict(desc=desc, fused_by_predicate=bool(F.series_pool_is_fused(layer._operand(dev), pool)), series_bytes=series.numel() * 4)
        grads = {}
        for train in (False, True):
            ms, peak = {k: [] for k, _ in sides}, {}
            for _ in range(args.repeats):               # alternating: both sides once per repeat
                for k, fn in sides:
                    step = step_of(fn, train)
                    ms[k].append(events_ms(step, args.steps, args.warmup))
                    clear()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    step()
                    torch.cuda.synchronize()
                    peak[k] = torch.cuda.max_memory_allocated() - base
                    if train:
                        grads[k] = [series.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
            col = {}
            for k, _ in sides:
                col[k] = dict(ms_per_call=ms[k], median=sorted(ms[k])[len(ms[k]) // 2], spread=round(max(ms[k]) - min(ms[k]), 4),
                              peak_bytes_above_baseline=peak[k])
            col["fused_over_composition_ms"] = round(col["fused"]["median"] / col["composition"]["median"], 3)
            col["fused_over_composition_peak"] = round(peak["fused"] / peak["composition"], 3)
            entry["forward_backward" if train else "forward"] = col
        if drop is None:
            with torch.no_grad():
                entry["results_equal"] = bool(torch.equal(fused(), composition()))
            entry["gradients_equal"] = all(bool(torch.equal(a, b)) for a, b in zip(grads["fused"], grads["composition"]))
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        grads.clear()
        clear()
        torch.cuda.empty_cache()

    op = dti148(dev)
    S, T, H, K = 8, 284, 15, 10
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 32, K, H).to(dev)
    case("a_dti148_1to32", "dti148 S=8 T=284 H=15 K=10 f=1 -> g=32, window-major", l1, torch.randn(S, op.n, T, device=dev), False)
    del l1
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, K, H).to(dev)
    case("a_dti148_32to64_series", "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64, series layout", l2, torch.randn(S, op.n, T, 32, device=dev), True)
    del l2
    n, row, col, val = synth.sheet_mesh(300, device=dev)
    opm = GraphOperand.from_coo(n, row, col, val, dev)
    lm = tgcn_amd.TGCNCheb_H(opm, 4, 32, 5, 15).to(dev)
    case("b_mesh90k_4to32", "sheet_mesh(300) n=%d S=1 T=75 H=15 K=5 f=4 -> g=32, window-major" % n, lm, torch.randn(1, n, 75, 4, device=dev), False)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                   "r18_series_relu_pool.json" if drop is None else "r22_series_relu_dropout_pool.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_chunk_relu_pool(args):
    dev = torch.device("cuda:0")
    pool, drop = args.relu_pool, args.dropout or 0.0
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               pool=pool, dropout=drop, time_chunks=list(args.time_chunk), cases={})
    torch.manual_seed(0)
    seed = torch.tensor([0x2468ACE13579BDF], dtype=torch.int64, device=dev)
    thr, scale = F.dropout_params(drop)

    def case(name, desc, layer, series, as_series):
        series = series.requires_grad_(True)
        N = layer.weight.shape[-1]

        def pool_pass(y):
            y3 = y if y.dim() == 3 else y.reshape(y.shape[0], y.shape[1], -1)
            z = F.ReluDropoutPoolFn.apply(y3, pool, N, seed, thr, scale) if drop else F.ReluPoolFn.apply(y3, pool)
            return z if y.dim() == 3 else z.view(y.shape[0], y.shape[1] // pool, y.shape[2], N)

        def fused_unchunked():
            if drop:
                return tgcn_amd.cheb_series_relu_dropout_pool(layer, series, p=drop, pool=pool, seed=seed, as_series=as_series, padding="causal")
            return tgcn_amd.cheb_series_relu_pool(layer, series, pool=pool, as_series=as_series, padding="causal")

        columns = [("fused_unchunked", fused_unchunked)]
        for tc in args.time_chunk:
            columns.append(("time_chunk_%d_then_pool_pass" % tc,
                            lambda tc=tc: pool_pass(layer.forward_series(series, as_series=as_series, padding="causal", time_chunk=tc))))
            columns.append(("chunked_pooled_%d" % tc,
                            lambda tc=tc: tgcn_amd.cheb_series_relu_pool_chunked(layer, series, time_chunk=tc, pool=pool, p=drop, seed=seed,
                                                                                 as_series=as_series)))

        def clear():
            layer.zero_grad(set_to_none=True)
            series.grad = None

        def step_of(fn):
            def step():
                clear()
                z = fn()
                z.backward(torch.ones_like(z))
            return step

        ms, peak = {k: [] for k, _ in columns}, {}
        for _ in range(args.repeats):               # alternating: every column once per repeat
            for k, fn in columns:
                step = step_of(fn)
                ms[k].append(events_ms(step, args.steps, args.warmup))
                clear()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - base
        with torch.no_grad():
            zs = [fn() for _, fn in columns]
        S, n, T = series.shape[:3]
        full = 4 * S * n * T * N
        entry = dict(desc=desc, fused_by_predicate=bool(F.series_pool_is_fused(layer._operand(dev), pool)), series_bytes=series.numel() * 4,
                     full_output_bytes=full, results_equal_to_fused_unchunked=[bool(torch.equal(z, zs[0])) for z in zs[1:]])
        for k, _ in columns:
            entry[k] = dict(ms_per_step=ms[k], median=sorted(ms[k])[len(ms[k]) // 2], spread=round(max(ms[k]) - min(ms[k]), 4),
                            peak_bytes_above_baseline=peak[k], peak_over_full_output=round(peak[k] / full, 4),
                            ms_over_fused_unchunked=round(sorted(ms[k])[len(ms[k]) // 2] / sorted(ms["fused_unchunked"])[len(ms[k]) // 2], 3))
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        del zs
        clear()
        torch.cuda.empty_cache()

    op = dti148(dev)
    S, T, H, K = 8, 284, 15, 10
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 32, K, H).to(dev)
    case("a_dti148_1to32", "dti148 S=8 T=284 H=15 K=10 f=1 -> g=32 causal, window-major, forward + backward", l1, torch.randn(S, op.n, T, device=dev), False)
    del l1
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, K, H).to(dev)
    case("a_dti148_32to64_series", "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64 causal, series layout, forward + backward", l2,
         torch.randn(S, op.n, T, 32, device=dev), True)
    del l2
    n, row, col, val = synth.sheet_mesh(300, device=dev)
    opm = GraphOperand.from_coo(n, row, col, val, dev)
    lm = tgcn_amd.TGCNCheb_H(opm, 4, 32, 5, 15).to(dev)
    case("b_mesh90k_4to32", "sheet_mesh(300) n=%d S=1 T=75 H=15 K=5 f=4 -> g=32 causal, window-major, forward + backward" % n, lm,
         torch.randn(1, n, 75, 4, device=dev), False)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r23_series_chunk_relu_pool.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main_fused_series(args):
    import inspect
    dev = torch.device("cuda:0")
    has_kw = "fused" in inspect.signature(tgcn_amd.TGCNCheb_H.forward_series).parameters
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               has_fused_keyword=has_kw, cases={})
    torch.manual_seed(0)

    def case(name, desc, layer, series, as_series):
        S, n, T, f = series.shape
        K, H, _, N = layer.weight.shape
        x = (series[..., 0] if f == 1 else series).contiguous().requires_grad_(True)       # a single channel is given as a 3-D series
        xw = windows(series, H).requires_grad_(True)         # the windows exist beforehand: cutting them is not timed
        entry = dict(desc=desc)
        fusable = False
        if has_kw:
            op = layer._operand(dev)
            fusable = F.series_fused_supported(op, f, H, N, K, T, 0, 1, F.MODE_POWER)
            rc, tb, dense, lds = F._series_small_plan(op, f, H, N, K, T, 0, 0, 1, F.MODE_POWER)
            entry["plan"] = dict(rc=rc, tb=tb, dense=dense, lds_bytes=lds, workgroups=S * -(-(T - H + 1) // tb) if rc == 0 else 0)
        columns = ["unfused"] + (["fused"] if fusable else []) + ["materialised"]

        def forward(col):
            if col == "materialised":
                return layer(xw)
            return layer.forward_series(x, as_series=as_series, **(dict(fused=True) if col == "fused" else {}))

        def step_of(col, train):
            def step():
                if not train:
                    with torch.no_grad():
                        forward(col)
                    return
                layer.zero_grad(set_to_none=True)
                x.grad = xw.grad = None
                out = forward(col)
                out.backward(torch.ones_like(out))
            return step

        if fusable:
            with torch.no_grad():
                a, b = forward("fused"), forward("unfused")
            entry["fused_vs_unfused_max_rel"] = float((a - b).abs().max() / b.abs().max())
        for train in (False, True):
            ms = {c: [] for c in columns}
            for _ in range(args.repeats):               # alternating: every column once per repeat
                for c in columns:
                    ms[c].append(events_ms(step_of(c, train), args.steps, args.warmup))
            entry["forward_backward" if train else "forward"] = {
                c: dict(ms_per_call=ms[c], median=sorted(ms[c])[len(ms[c]) // 2], spread=round(max(ms[c]) - min(ms[c]), 4)) for c in columns}
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        layer.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()

    op = dti148(dev)
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 32, 10, 15).to(dev)
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, 10, 15).to(dev)
    x1, x32 = torch.randn(8, op.n, 284, 1, device=dev), torch.randn(8, op.n, 284, 32, device=dev)
    for as_series in (False, True):
        tag = "series" if as_series else "windows"
        case("a_dti148_1to32_" + tag, "dti148 S=8 T=284 H=15 K=10 f=1 -> g=32, as_series=%s" % as_series, l1, x1, as_series)
        case("a_dti148_32to64_" + tag, "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64, as_series=%s" % as_series, l2, x32, as_series)
    del l1, l2, x1, x32
    n, row, col, val = synth.grid_knn(28, device=dev)
    opg = GraphOperand.from_coo(n, row, col, val, dev)
    lg = tgcn_amd.TGCNCheb_H(opg, 1, 64, 5, 28).to(dev)
    case("g_grid784_1to64", "grid_knn(28) n=784 S=8 T=128 H=28 K=5 f=1 -> g=64, window-major", lg, torch.randn(8, n, 128, 1, device=dev), False)
    for item in args.include:
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        rel = {name: {m: round(entry[m]["unfused"]["median"] / res["cases"][name][m]["unfused"]["median"], 3) for m in ("forward", "forward_backward")}
               for name, entry in other["cases"].items() if name in res["cases"]}
        res.setdefault("runs", {})[label] = dict(run=other, unfused_ms_over_this_run=rel)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r21_series_small.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def series_pool_auto_classes(rows):
    """F.SERIES_POOL_FUSED_AUTO's rule on this run's rows: a class is listed only where the one-launch call's median lies below BOTH
    comparators' by more than the largest of the three spreads, in every row of the class"""
    out = []
    for klass in ("pool", "pool_dropout"):
        mine = [r for r in rows if r["class"] == klass and r.get("label") == "this" and "fused" in r]
        if mine and all(r["fused"]["median_ms"] + max(r[c]["spread_ms"] for c in ("fused", "general", "composed"))
                        < min(r["general"]["median_ms"], r["composed"]["median_ms"]) for r in mine):
            out.append(klass)
    return out


def main_fused_series_pool(args):
    """--fused-series --relu-pool P [--dropout PROB]: relu (+ dropout) + pool behind the one-launch series layer"""
    dev = torch.device("cuda:0")
    has_new = hasattr(tgcn_amd, "cheb_series_relu_pool_fused")
    pool, drop = args.relu_pool, args.dropout or 0.0
    klass = "pool_dropout" if drop else "pool"
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               pool=pool, dropout=drop, has_fused_pool_call=has_new, rows=[])
    torch.manual_seed(0)
    seed = torch.tensor([20240], dtype=torch.int64, device=dev)
    thr, scale = F.dropout_params(drop)

    def case(name, desc, layer, series):
        x = series.contiguous().requires_grad_(True)

        def forward(col):
            if col == "fused":         # (a) the new call
                return tgcn_amd.cheb_series_relu_pool_fused(layer, x, pool=pool, p=drop, seed=seed, fused=True)
            if col == "general":       # (b) the general pooled epilogue
                if drop:
                    return tgcn_amd.cheb_series_relu_dropout_pool(layer, x, p=drop, pool=pool, seed=seed)
                return tgcn_amd.cheb_series_relu_pool(layer, x, pool=pool)
            y = layer.forward_series(x, fused=True)      # (c) the one-launch layer, then the relu (+ dropout) + pool pass
            return F._relu_dropout_pool_view(y, pool, seed, thr, scale) if drop else F._relu_pool_view(y, pool)

        def step_of(col, train):
            def step():
                if not train:
                    with torch.no_grad():
                        forward(col)
                    return
                layer.zero_grad(set_to_none=True)
                x.grad = None
                z = forward(col)
                z.backward(torch.ones_like(z))
            return step

        columns = (["fused"] if has_new else []) + ["general", "composed"]
        equal = None
        if has_new:
            with torch.no_grad():
                equal = bool(torch.equal(forward("fused"), forward("composed")))
        for train in (False, True):
            ms = {c: [] for c in columns}
            for _ in range(args.repeats):               # alternating: every column once per repeat
                for c in columns:
                    ms[c].append(events_ms(step_of(c, train), args.steps, args.warmup))
            row = dict(case=name, desc=desc, direction="forward_backward" if train else "forward", label="this", fused_equals_composed=equal)
            row["class"] = klass
            for c in columns:
                row[c] = dict(ms_per_call=ms[c], median_ms=sorted(ms[c])[len(ms[c]) // 2], spread_ms=round(max(ms[c]) - min(ms[c]), 4))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        layer.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()

    op = dti148(dev)
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 32, 10, 15).to(dev)
    case("a_dti148_1to32", "dti148 S=8 T=284 H=15 K=10 f=1 -> g=32, window-major, pool %d%s" % (pool, ", p=%g" % drop if drop else ""), l1,
         torch.randn(8, op.n, 284, device=dev))
    del l1
    n, row, col, val = synth.grid_knn(28, device=dev)
    opg = GraphOperand.from_coo(n, row, col, val, dev)
    lg = tgcn_amd.TGCNCheb_H(opg, 1, 64, 5, 28).to(dev)
    case("g_grid784_1to64", "grid_knn(28) n=784 S=8 T=128 H=28 K=5 f=1 -> g=64, window-major, pool %d%s" % (pool, ", p=%g" % drop if drop else ""), lg,
         torch.randn(8, n, 128, device=dev))
    for item in args.include:       # another run's file: its rows under LABEL (the parent's build: comparators only), and the rule over all
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        res["rows"] += [dict(r, label=label) if r.get("label") == "this" else r for r in other["rows"]]
    res["auto"] = dict(rule="a class is listed only where fused.median_ms + max(spread_ms of fused, general, composed) < min(general.median_ms, "
                            "composed.median_ms) in every row labelled 'this' of the class", classes=series_pool_auto_classes(res["rows"]))
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r24_series_small_pool.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def stride_arg(text):
    parts = tuple(int(v) for v in text.split(","))
    return parts[0] if len(parts) == 1 else parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32", help="bf16: the bfloat16 streaming cases (profiles/r10_series_bf16.json)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stride", type=stride_arg, default=1, help="the window step; with --stream: S1,S2,S3, the three layers' steps")
    ap.add_argument("--repeats", type=int, default=3, help="with --stream --stride and --time-chunk: event timings per column")
    ap.add_argument("--padding", type=padding_arg, default=0)
    ap.add_argument("--conv", action="store_true", help="add the stride-4 and causal-chain cases")
    ap.add_argument("--dilation", action="store_true", help="the dilated cases (profiles/r11_series_dilation.json)")
    ap.add_argument("--stream", action="store_true", help="the streaming-state cases (profiles/r12_series_stream.json)")
    ap.add_argument("--graph", action="store_true", help="with --stream: the captured step next to the eager one (profiles/r13_series_stream_graph.json)")
    ap.add_argument("--fused", action="store_true", help="with --stream: the one-launch step next to the eager one (profiles/r14_series_stream_fused.json)")
    ap.add_argument("--time-chunk", type=lambda t: tuple(int(v) for v in t.split(",")), default=None, metavar="Tc[,Tc...]",
                    help="a training step on T = 1200, unchunked against each time_chunk (profiles/r17_series_time_chunk.json)")
    ap.add_argument("--relu-pool", type=int, choices=(2, 4), default=None, metavar="P",
                    help="cheb_series_relu_pool against gcn_pool_4(relu(forward_series)) on the same commit (profiles/r18_series_relu_pool.json)")
    ap.add_argument("--dropout", type=float, default=None, metavar="PROB",
                    help="with --relu-pool P: cheb_series_relu_dropout_pool against forward_series -> relu -> dropout -> pool and against "
                         "cheb_series_relu_pool (profiles/r22_series_relu_dropout_pool.json)")
    ap.add_argument("--fused-series", action="store_true",
                    help="forward_series(fused=True) next to the unfused call and the materialised windows (profiles/r21_series_small.json)")
    ap.add_argument("--include", action="append", default=[], metavar="LABEL=FILE",
                    help="put another run's --out file (the parent commit's, a repeat of this one) into this one under runs[LABEL], with "
                         "each shared case's ms per call relative to this run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.dropout is not None and (args.relu_pool is None or not 0.0 < args.dropout < 1.0):
        ap.error("--dropout PROB (0 < PROB < 1) goes with --relu-pool P")
    if args.dtype == "bf16":
        return main_bf16(args)
    if args.fused_series:
        if args.time_chunk is not None or args.stream or args.dilation or args.conv:
            ap.error("--fused-series runs alone or with --relu-pool P [--dropout PROB]")
        return main_fused_series_pool(args) if args.relu_pool is not None else main_fused_series(args)
    if args.relu_pool is not None and args.time_chunk is not None:
        if min(args.time_chunk) < 1 or args.stream or args.dilation or args.conv:
            ap.error("--time-chunk Tc[,Tc...] (integers >= 1) --relu-pool P [--dropout PROB] run without the other case switches")
        return main_chunk_relu_pool(args)
    if args.relu_pool is not None:
        if args.stream or args.dilation or args.conv:
            ap.error("--relu-pool P runs alone or with --time-chunk")
        return main_relu_pool(args)
    if args.time_chunk is not None:
        if min(args.time_chunk) < 1 or args.stream or args.dilation or args.conv:
            ap.error("--time-chunk Tc[,Tc...] (integers >= 1) runs alone")
        return main_time_chunk(args)
    if args.dilation:
        return main_dilation(args)
    if args.graph and not args.stream:
        ap.error("--graph goes with --stream")
    if args.fused and not args.stream:
        ap.error("--fused goes with --stream")
    if isinstance(args.stride, tuple):
        if not args.stream or args.graph or args.fused or len(args.stride) != 3 or min(args.stride) < 1:
            ap.error("--stride S1,S2,S3 (three steps >= 1) goes with --stream alone")
        return main_stream_stride(args)
    if args.stream and args.fused:
        return main_stream_fused(args)
    if args.stream and args.graph:
        return main_stream_graph(args)
    if args.stream:
        return main_stream(args)
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, warmup=args.warmup, stride=args.stride,
               padding=args.padding, cases={})
    torch.manual_seed(0)

    def case(name, desc, layer, series, H, stride=args.stride, padding=args.padding):
        series = series.requires_grad_(True)
        xw = windows(series.detach(), H, stride, padding).requires_grad_(True)
        geo = {} if (stride, padding) == (1, 0) else dict(stride=stride, padding=padding)      # the default call exactly as it was
        if geo:
            desc += " stride=%s padding=%s" % (stride, padding)
        entry = dict(desc=desc, **compare(lambda: layer.forward_series(series, **geo), lambda: layer(xw), args.steps, args.warmup))
        res["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        del xw
        torch.cuda.empty_cache()

    op = dti148(dev)
    S, T, H, K = 8, 284, 15, 10
    l1 = tgcn_amd.TGCNCheb_H(op, 1, 32, K, H).to(dev)
    l2 = tgcn_amd.TGCNCheb_H(op, 32, 64, K, H).to(dev)
    case("a_dti148_1to32", "dti148 S=8 T=284 H=15 K=10 f=1 -> g=32", l1, torch.randn(S, op.n, T, 1, device=dev), H)
    case("a_dti148_32to64", "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64", l2, torch.randn(S, op.n, T, 32, device=dev), H)
    if args.conv:
        case("a_dti148_32to64_stride4", "dti148 S=8 T=284 H=15 K=10 f=32 -> g=64", l2, torch.randn(S, op.n, T, 32, device=dev), H, 4, 0)

    n, row, col, val = synth.sheet_mesh(300, device=dev)
    opm = GraphOperand.from_coo(n, row, col, val, dev)
    lm = tgcn_amd.TGCNCheb_H(opm, 4, 32, 5, 15).to(dev)
    case("b_mesh90k_4to32", "sheet_mesh(300) n=%d S=1 T=75 H=15 K=5 f=4 -> g=32" % n, lm, torch.randn(1, n, 75, 4, device=dev), 15)
    if args.conv:
        case("b_mesh90k_4to32_stride4", "sheet_mesh(300) n=%d S=1 T=75 H=15 K=5 f=4 -> g=32" % n, lm, torch.randn(1, n, 75, 4, device=dev), 15, 4, 0)
    del lm, opm
    torch.cuda.empty_cache()

    series = torch.randn(S, op.n, T, 1, device=dev).requires_grad_(True)
    xw1 = windows(series.detach(), H).requires_grad_(True)
    T1 = T - H + 1

    def chain_stream():
        return l2.forward_series(torch.relu(l1.forward_series(series, as_series=True)))

    def chain_batch():
        h = torch.relu(l1(xw1))                                           # (S*T1, n, 32)
        return l2(windows(h.view(S, T1, op.n, 32).permute(0, 2, 1, 3), H))
    entry = dict(desc="dti148 S=8 T=284: TGCNCheb_H(1,32,10,15) -> relu -> TGCNCheb_H(32,64,10,15)", **compare(chain_stream, chain_batch, args.steps, args.warmup))
    res["cases"]["c_dti148_chain"] = entry
    print(json.dumps({"c_dti148_chain": entry}), flush=True)
    if args.conv:
        del xw1
        torch.cuda.empty_cache()
        xc1 = windows(series.detach(), H, 1, "causal").requires_grad_(True)              # (S*T, n, H, 1)

        def causal_stream():
            return l2.forward_series(torch.relu(l1.forward_series(series, as_series=True, padding="causal")), padding="causal")

        def causal_batch():
            h = torch.relu(l1(xc1))                                       # (S*T, n, 32)
            return l2(windows(h.view(S, T, op.n, 32).permute(0, 2, 1, 3), H, 1, "causal"))
        entry = dict(desc='dti148 S=8 T=284: the chain with padding="causal" in both layers, 284 windows out',
                     **compare(causal_stream, causal_batch, args.steps, args.warmup))
        res["cases"]["c_dti148_chain_causal"] = entry
        print(json.dumps({"c_dti148_chain_causal": entry}), flush=True)
    for item in args.include:
        label, path = item.split("=", 1)
        with open(path) as f:
            other = json.load(f)
        rel = {}
        for name, entry in other["cases"].items():
            if name in res["cases"]:
                rel[name] = {d: {k: round(entry[d][k]["ms_per_call"] / res["cases"][name][d][k]["ms_per_call"], 3) for k in ("streaming", "materialised")}
                             for d in ("forward", "forward_backward")}
        res.setdefault("runs", {})[label] = dict(run=other, ms_over_this_run=rel)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
