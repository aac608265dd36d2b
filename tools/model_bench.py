#!/usr/bin/env python3
"""One training step (forward, backward, SGD) of a model written like the reference's HCP network
(examples/pytorch_based/pytorch_hcp_tgcn.py:93-155: TGCNCheb_H(L0,1,32,10,15) -> relu -> gcn_pool_4 ->
GCNCheb(L2,32,64,10) -> relu -> gcn_pool_4 -> linear) at batch 512 on the 148-parcel graph, with the layers imported
through the compat path.  Developer tool: the number a user of the reference sees after switching.

    python tools/model_bench.py [--batch 512] [--steps 100] [--fused] [--graph] [--time-chunk 32] [--repeats 3] [--json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "compat"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as TF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--fused", action="store_true", help="use tgcn_amd.cheb_relu_pool for layer + relu + pool")
    ap.add_argument("--graph", action="store_true", help="replay the training step from one hipGraph (tgcn_amd.GraphedTrainStep)")
    ap.add_argument("--copy-batch", action="store_true", help="with --graph: pass a batch that is copied into the static buffers on every call")
    ap.add_argument("--time-chunk", type=int, default=0, help="time the chunked 148-parcel layer (1 -> 32 channels, S=8, T=284) at this time_chunk instead of the model")
    ap.add_argument("--repeats", type=int, default=1, help="timed repeats of --steps steps each; the median is printed")
    ap.add_argument("--json", action="store_true", help="also print one JSON line with every repeat")
    args = ap.parse_args()
    from tgcn.nn.gcn import GCNCheb, TGCNCheb_H, gcn_pool_4           # the reference's import line
    import tgcn_amd
    z = np.load(os.path.join(ROOT, "tests", "golden", "TGCNChebH_dti148_q4_f1_g32_K10_H15.npz"))
    n = n0 = int(z["n"])
    import scipy.sparse as sp
    L0 = torch.tensor(sp.csr_matrix((z["val"], z["col"], z["rowptr"]), shape=(n, n)).toarray(), dtype=torch.float32)
    pad = (-n) % 16                                    # the reference's coarsening pads with isolated vertices (gcn/coarsening.py)
    L0 = TF.pad(L0, (0, pad, 0, pad))
    n += pad
    rng = np.random.default_rng(0)
    n2 = n // 4
    A = (rng.random((n2, n2)) < 0.5).astype(np.float32)
    A = np.triu(A, 1)
    A = A + A.T
    dis = 1.0 / np.sqrt(np.maximum(A.sum(0), 1))
    L2 = torch.tensor(-(dis[:, None] * A * dis[None, :]), dtype=torch.float32)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.tgcn1 = TGCNCheb_H(L0, 1, 32, 10, 15)
            self.gcn2 = GCNCheb(L2, 32, 64, 10)
            self.fc = nn.Linear((n2 // 4) * 64, 6)

        def forward(self, x):
            if args.fused:
                x = tgcn_amd.cheb_relu_pool(self.tgcn1, x, pool=4)
                x = tgcn_amd.cheb_relu_pool(self.gcn2, x, pool=4)
            else:
                x = gcn_pool_4(TF.relu(self.tgcn1(x)))
                x = gcn_pool_4(TF.relu(self.gcn2(x)))
            return TF.log_softmax(self.fc(x.reshape(x.shape[0], -1)), dim=1)

    class ChunkNet(nn.Module):
        """the launch-bound chunked layer of profiles/r23_series_chunk_relu_pool.json (case a_dti148_1to32): 1 -> 32 channels on the 148
        parcels, relu + dropout + pool in the epilogue, walked args.time_chunk time rows at a time; a linear head per time row"""

        def __init__(self):
            super().__init__()
            self.tgcn1 = TGCNCheb_H(L0[:n0, :n0].contiguous(), 1, 32, 10, 15)
            self.fc = nn.Linear((n0 // 4) * 32, 6)

        def forward(self, series):
            z = tgcn_amd.cheb_series_relu_pool_chunked(self.tgcn1, series, time_chunk=args.time_chunk, pool=4, p=0.1)
            return TF.log_softmax(self.fc(z.reshape(z.shape[0], -1)), dim=1)

    torch.manual_seed(0)
    if args.time_chunk:
        net = ChunkNet().cuda()
        x = torch.randn(8, n0, 284, device="cuda")
        y = torch.randint(0, 6, (8 * 284,), device="cuda")
        what = "148-parcel chunked layer 1 -> 32, S=8 T=284, time_chunk %d" % args.time_chunk
    else:
        net = Net().cuda()
        x = torch.randn(args.batch, n, 15, device="cuda")
        y = torch.randint(0, 6, (args.batch,), device="cuda")
        what = "HCP-style model, batch %d, %s" % (args.batch, "fused relu+pool" if args.fused else "plain modules")
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = TF.nll_loss(net(x), y)
        loss.backward()
        opt.step()
        return loss

    if args.graph:
        gts = tgcn_amd.GraphedTrainStep(net, opt, TF.nll_loss, x, y, warmup=5)

        # the example objects themselves are not copied again (a replay alone, what a hand-written capture times); --copy-batch passes other
        # tensors, which are copied into the static buffers on every call, as a training loop's batches are
        xb, yb = (x.clone(), y.clone()) if args.copy_batch else (x, y)

        def step():      # noqa: F811 -- the same step, replayed
            return gts(xb, yb)

    def timed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, loss

    for _ in range(10):
        step()
    times = []
    for _ in range(args.repeats):
        dt, loss = timed()
        times.append(dt * 1e3)
    dt = sorted(times)[len(times) // 2] * 1e-3
    net.eval()
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            net(x)
        torch.cuda.synchronize()
        df = (time.perf_counter() - t0) / args.steps
    print("%s%s: inference %.3f ms, training step %.3f ms (%.0f samples/s), loss %.4f" % (
        what, ", step replayed by GraphedTrainStep" if args.graph else "", df * 1e3, dt * 1e3, x.shape[0] / dt, float(loss.detach())), flush=True)
    if args.json:
        print(json.dumps({"case": what, "graph": bool(args.graph), "copy_batch": bool(args.graph and args.copy_batch),"steps": args.steps, "ms_per_step": [round(t, 4) for t in times],
                          "median": round(dt * 1e3, 4), "spread": round(max(times) - min(times), 4), "inference_ms": round(df * 1e3, 4)}), flush=True)


if __name__ == "__main__":
    main()
