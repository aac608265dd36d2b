#!/usr/bin/env python3
"""The same layer with fp32 and with bfloat16 parameters: ms per call and per kernel kind (tgcn_profile_*), and the hop's algorithmic bytes
against the 8 TB/s HBM peak computed as bench.py's `roofline` block does (8 B per stored entry, 4 B per row pointer, a read and a write
of every row element per hop: 4 + 4 B in fp32, 2 + 2 B in bf16).  Developer tool; the benchmark metric stays bench.py's fp32 headline.

    python tools/precision_bench.py [--steps 5] [--warmup 2] [--out profiles/r07_bf16_precision.json]

Cases: cfg4 (sheet mesh n = 90 k, TGCNCheb_H(L, 1, 32, 5, 1200), q = 1: the project-first path) forward and forward + backward; an
R-MAT at reduced scale (n = 2 M, nnz = 32 M, C = 64 -> 64, K = 5, 16 time steps: the hops path) forward, fp32 on the uncompacted
operand too, so that both dtypes' hops run over the same rows.

On the R-MAT case the bf16 layer is also timed on compact hop tensors against full-size ones (F.COMPACT_BF16 on / off) in the same process,
alternating, three repeats each: median and max - min of the ms per call, the per-kind kernel times of each setting's median repeat, and
torch.equal of the two outputs -> --compact-out (profiles/r15_bf16_compact.json).  --only-compact runs nothing else."""
import argparse
import collections
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tgcn_amd import _lib, functional as F  # noqa: E402
from tgcn_amd.graph import GraphOperand  # noqa: E402
from tools import synth  # noqa: E402

KINDS = {0: "hop", 1: "hop_fixup", 2: "project", 3: "relayout", 4: "small", 5: "wgrad", 6: "small_basis", 7: "hop_long", 8: "project_gather"}
HBM_PEAK_GBPS = 8000.0


def measure(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    _lib.profile_start(1 << 16)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    prof = _lib.profile_stop(1 << 16)
    by = collections.defaultdict(list)
    for kind, ms in prof:
        by[KINDS.get(kind, str(kind))].append(ms)
    return dict(ms_per_call=round(a.elapsed_time(b) / steps, 4),
                kernel_ms_per_call={k: round(sum(v) / steps, 4) for k, v in sorted(by.items())},
                launches_per_call={k: len(v) // steps for k, v in sorted(by.items())},
                mean_launch_ms={k: round(float(np.mean(v)), 4) for k, v in sorted(by.items())}), by


def hop_roofline(op, K, F_cols, elem_bytes, hop_ms, steps):
    """bench.py's hop roofline over one forward: (K - 1) hops of 8 nnz + 4 (n + 1) + 2 * elem_bytes * n * F bytes (F = every time step's
    row elements: the fp32 path may issue a launch per time step where the bf16 path issues one for all of them) against the forward's
    hop time"""
    if not hop_ms:
        return None
    per_fwd = (K - 1) * (8 * op.nnz + 4 * (op.n + 1) + 2 * elem_bytes * op.n * F_cols)
    ms = float(np.sum(hop_ms)) / steps
    ach = per_fwd / (ms * 1e-3) / 1e9
    return dict(algorithmic_bytes_per_forward=int(per_fwd), hop_ms_per_forward=round(ms, 4), launches_per_forward=len(hop_ms) // steps,
                achieved_GBps=round(ach, 1), peak_GBps=HBM_PEAK_GBPS, frac=round(ach / HBM_PEAK_GBPS, 4))


def run_layer(op, x, W, bias, kind, mode, train):
    def fn():
        if train:
            Wp, bp, xp = W.detach().requires_grad_(True), bias.detach().requires_grad_(True), x.detach().requires_grad_(True)
            F.cheb_layer(op, xp, Wp, bp, kind, mode).backward(torch.ones((x.shape[0], x.shape[1], W.shape[2]), dtype=W.dtype, device=x.device))
        else:
            with torch.no_grad():
                F.cheb_layer(op, x, W, bias, kind, mode)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rmat-n", type=int, default=2_000_000)
    ap.add_argument("--rmat-nnz", type=int, default=32_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--compact-out", default=None)
    ap.add_argument("--only-compact", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lib_hash=_lib.binary_hash(), steps=args.steps, cases={})
    if not args.only_compact:
        cfg4_case(args, dev, res)
    rmat_case(args, dev, res)
    if args.out and not args.only_compact:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def cfg4_case(args, dev, res):
    # cfg4: the project-first path (2 N <= C): the hops run on the fp32 projection in both dtypes
    n, row, col, val = synth.sheet_mesh(300, device=dev)
    op = GraphOperand.from_coo(n, row, col, val, dev)
    torch.manual_seed(0)
    x = torch.randn(1, n, 1200, device=dev)
    W = torch.empty(5, 1200, 32, device=dev).uniform_(-0.013, 0.013)
    b = torch.empty(n, 32, device=dev).uniform_(-0.013, 0.013)
    for train in (False, True):
        entry = {}
        for dt in (torch.float32, torch.bfloat16):
            r, by = measure(run_layer(op, x, W.to(dt), b.to(dt), F.BIAS_VERTEX_CHANNEL, F.MODE_POWER, train), args.steps, args.warmup)
            r["hop_roofline"] = hop_roofline(op, 5, 32, 4, by.get("hop"), args.steps)      # Z and the hops are fp32 in both
            if train:
                r["note"] = "kernel times cover the forward only: the backward runs on autograd's thread, which the thread-local launch record does not see"
            entry[str(dt).replace("torch.", "")] = r
        res["cases"]["cfg4_" + ("forward_backward" if train else "forward")] = entry
        print(json.dumps({"cfg4_" + ("fwd_bwd" if train else "fwd"): entry}), flush=True)
    del x, W, b, op
    torch.cuda.empty_cache()


def compact_bf16_case(args, op, x, W, b, desc):
    """the bf16 layer with F.COMPACT_BF16 on and off, alternating, three repeats each (the yardstick is the uncompacted path of this run)"""
    plan = op.compact_plan("rows")
    runs = {True: [], False: []}
    outs = {}
    saved = F.COMPACT_BF16
    try:
        for rep in range(3):
            for on in (True, False):
                F.COMPACT_BF16 = on
                r, _ = measure(run_layer(op, x, W, b, F.BIAS_VERTEX_CHANNEL, F.MODE_POWER, False), args.steps, args.warmup)
                runs[on].append(r)
        for on in (True, False):
            F.COMPACT_BF16 = on
            with torch.no_grad():
                outs[on] = F.cheb_layer(op, x, W, b, F.BIAS_VERTEX_CHANNEL, F.MODE_POWER)
    finally:
        F.COMPACT_BF16 = saved

    def summary(rs):
        ms = sorted(r["ms_per_call"] for r in rs)
        mid = sorted(rs, key=lambda r: r["ms_per_call"])[1]
        return dict(ms_per_call=[r["ms_per_call"] for r in rs], median_ms=ms[1], spread_ms=round(ms[-1] - ms[0], 4),
                    kernel_ms_per_call=mid["kernel_ms_per_call"], launches_per_call=mid["launches_per_call"], mean_launch_ms=mid["mean_launch_ms"])
    on, off = summary(runs[True]), summary(runs[False])
    gain = off["median_ms"] - on["median_ms"]
    return dict(desc=desc, plan=None if plan is None else dict(n=plan.n, n_c=plan.n_c, n_empty=plan.n_empty,
                                                               hop_tensor_share_left_out=round(plan.n_empty / plan.n, 4)),
                compact_bf16_on=on, compact_bf16_off=off, median_gain_ms=round(gain, 4),
                faster_beyond_spread=bool(gain > max(on["spread_ms"], off["spread_ms"])),
                outputs_equal=bool(torch.equal(outs[True], outs[False])))


def rmat_case(args, dev, res):
    # R-MAT at reduced scale: the hops path, fp32 uncompacted and bf16 over the same rows
    n, row, col, val = synth.rmat(args.rmat_n, args.rmat_nnz, seed=12345, labeling="random", device=dev)
    op = GraphOperand.from_coo(n, row, col, val, dev)
    del row, col, val
    q, C, N, K = 16, 64, 64, 5
    x = torch.randn(q, n, C, device=dev)
    W = torch.empty(K, C, N, device=dev).uniform_(-0.056, 0.056)
    b = torch.empty(n, N, device=dev).uniform_(-0.056, 0.056)
    entry = dict(desc="R-MAT n=%d nnz=%d random labels, TGCNCheb(L,64,64,5), q=16" % (n, op.nnz))
    if args.compact_out:
        BF = torch.bfloat16
        cres = dict(device=res["device"], lib_hash=res["lib_hash"], steps=args.steps, warmup=args.warmup,
                    case=compact_bf16_case(args, op, x.to(BF), W.to(BF), b.to(BF), entry["desc"] + ", bf16 forward"))
        print(json.dumps({"rmat_bf16_compact": cres["case"]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.compact_out)), exist_ok=True)
        with open(args.compact_out, "w") as f:
            json.dump(cres, f, indent=1)
    if args.only_compact:
        return
    for label, dt, compact in (("float32_compact", torch.float32, True), ("float32", torch.float32, False), ("bfloat16", torch.bfloat16, False)):
        F.COMPACT = compact
        try:
            r, by = measure(run_layer(op, x.to(dt) if dt != torch.float32 else x, W.to(dt), b.to(dt), F.BIAS_VERTEX_CHANNEL, F.MODE_POWER, False),
                            args.steps, args.warmup)
        finally:
            F.COMPACT = True
        if not compact:
            r["hop_roofline"] = hop_roofline(op, K, q * C, 2 if dt == torch.bfloat16 else 4, by.get("hop"), args.steps)
        entry[label] = r
    h32, h16 = entry["float32"]["hop_roofline"], entry["bfloat16"]["hop_roofline"]
    if h32 and h16:
        entry["bf16_over_fp32_hop_time"] = round(h16["hop_ms_per_forward"] / h32["hop_ms_per_forward"], 3)
    res["cases"]["rmat_reduced_forward"] = entry
    print(json.dumps({"rmat_reduced_forward": entry}), flush=True)


if __name__ == "__main__":
    main()
