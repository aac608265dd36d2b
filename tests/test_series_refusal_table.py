"""What every exported entry of the streaming time-window family answers to a grid of argument tuples, against the answers recorded
from the ABI 8 library before its host side was rebuilt around one geometry, one parameter builder and three drivers
(tests/golden/series_refusals_abi8.json, written by `tools/make_golden.py --series-refusals`).

CPU only.  The data pointers are never read: without a device an accepted call fails at its first launch (TGCN_ERR_LAUNCH, -2) and a
refused one returns TGCN_ERR_INVALID (-1), TGCN_ERR_WORKSPACE (-3) or TGCN_ERR_UNSUPPORTED (-4) before it.  A workspace query's row is
the byte count, a plan's row the triple (rc, hc, lds_bytes).

The grid: one valid base shape per entry (S=2, n=48, T=20 or Tc=5, f=4, H=3, N=8, K=3), one argument moved at a time through VALUES,
and the combinations of COMBOS.  Rows are only ever added: the recording is regenerated from the ABI 8 library, never edited."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "series_refusals_abi8.json")
BIG = 2 ** 31 - 1
POINTERS = ("stack", "W", "bias", "out", "idx", "ring", "pos", "g", "G", "dW")       # 1: the never-read pointer, 0: null
_SHAPE = ["S", "n", "T", "f", "H", "N", "K"]
_FWD = _SHAPE + ["stack", "W", "bias", "bias_kind"]
_FWD_B = _SHAPE + ["stack", "stack_ld", "W", "bias", "bias_dtype", "bias_kind"]
_BWD = _SHAPE + ["stack", "g", "g_as_series", "W", "G", "dW", "ws", "ws_bytes"]
_BWD_B = _SHAPE + ["stack", "stack_ld", "g", "g_as_series", "W", "G", "dW", "ws", "ws_bytes"]
_CONV = ["stride", "pl", "pr"]

# entry -> (argument names in the C order behind the stream, the matching workspace query or None)
ENTRIES = {
    "tgcn_cheb_project_series_f32": (_FWD + ["as_series", "out"], None),
    "tgcn_cheb_project_series_conv_f32": (_FWD + ["as_series", "out"] + _CONV, None),
    "tgcn_cheb_project_series_dilated_f32": (_FWD + ["as_series", "out"] + _CONV + ["dil"], None),
    "tgcn_cheb_project_series_pool_f32": (_FWD + ["as_series", "out", "idx", "pool"] + _CONV + ["dil"], None),
    "tgcn_cheb_project_series_stream_f32": (_FWD + ["out", "ring", "ring_ld", "head", "dil"], None),
    "tgcn_cheb_project_series_stream_pos_f32": (_FWD + ["out", "ring", "ring_ld", "pos", "dil"], None),
    "tgcn_cheb_project_series_stream_pool_f32": (_FWD + ["out", "pool", "ring", "ring_ld", "head", "pos", "dil"], None),
    "tgcn_cheb_project_series_stream_at_f32": (_FWD + ["out", "out_T", "out_t0", "as_series", "ring", "ring_ld", "head", "dil"], None),
    "tgcn_cheb_project_series_stream_strided_f32": (_FWD + ["out", "ring", "ring_ld", "head", "pos", "stride", "win_off"], None),
    "tgcn_cheb_series_backward_f32": (_BWD, "tgcn_cheb_series_backward_workspace_bytes"),
    "tgcn_cheb_series_conv_backward_f32": (_BWD + _CONV, "tgcn_cheb_series_conv_backward_workspace_bytes"),
    "tgcn_cheb_series_dilated_backward_f32": (_BWD + _CONV + ["dil"], "tgcn_cheb_series_dilated_backward_workspace_bytes"),
    "tgcn_cheb_series_chunk_backward_f32": (_SHAPE + ["stack", "ring", "ring_ld", "head", "g", "out_T", "out_t0", "g_as_series", "W", "G", "dW", "ws",
                                                      "ws_bytes", "dil"], "tgcn_cheb_series_chunk_backward_workspace_bytes"),
    "tgcn_cheb_project_series_conv_bf16": (_FWD_B + ["as_series", "out"] + _CONV, None),
    "tgcn_cheb_project_series_dilated_bf16": (_FWD_B + ["as_series", "out"] + _CONV + ["dil"], None),
    "tgcn_cheb_project_series_stream_bf16": (_FWD_B + ["out", "ring", "ring_ld", "head", "dil"], None),
    "tgcn_cheb_project_series_stream_pos_bf16": (_FWD_B + ["out", "ring", "ring_ld", "pos", "dil"], None),
    "tgcn_cheb_project_series_stream_strided_bf16": (_FWD_B + ["out", "ring", "ring_ld", "head", "pos", "stride", "win_off"], None),
    "tgcn_cheb_series_conv_backward_bf16": (_BWD_B + _CONV, "tgcn_cheb_series_conv_backward_bf16_workspace_bytes"),
    "tgcn_cheb_series_dilated_backward_bf16": (_BWD_B + _CONV + ["dil"], "tgcn_cheb_series_dilated_backward_bf16_workspace_bytes"),
    "tgcn_series_stream_advance": (["pos", "T", "C"], None),
}
QUERIES = {       # workspace queries: no stream, the value is the row
    "tgcn_cheb_series_backward_workspace_bytes": _SHAPE,
    "tgcn_cheb_series_conv_backward_workspace_bytes": _SHAPE + _CONV,
    "tgcn_cheb_series_dilated_backward_workspace_bytes": _SHAPE + _CONV + ["dil"],
    "tgcn_cheb_series_chunk_backward_workspace_bytes": _SHAPE + ["dil"],
    "tgcn_cheb_series_conv_backward_bf16_workspace_bytes": _SHAPE + _CONV,
    "tgcn_cheb_series_dilated_backward_bf16_workspace_bytes": _SHAPE + _CONV + ["dil"],
}
PLANS = {         # (rc, hc, lds_bytes); "hc" / "lds" 0: a null result pointer
    "tgcn_series_gemm_plan": ["H", "f", "N", "vec"],
    "tgcn_series_conv_plan": ["H", "f", "N", "vec", "stride"],
    "tgcn_series_conv_plan_bf16": ["H", "f", "N", "vec", "stride"],
    "tgcn_series_pool_plan": ["H", "f", "N", "vec", "stride", "pool"],
}
CHUNKED = ("_stream", "_chunk_", "_advance")       # entries whose T is a chunk of Tc = 5 rows behind a ring of C = 2

BASE = dict(S=2, n=48, T=20, f=4, H=3, N=8, K=3, stack=1, W=1, bias=0, bias_kind=0, bias_dtype=0, as_series=1, g_as_series=1, out=1, idx=1, pool=4,
            stride=1, pl=0, pr=0, dil=1, ring=1, ring_ld=8, head=0, pos=1, out_T=20, out_t0=5, win_off=0, g=1, G=1, dW=1, ws="ok", ws_bytes=None,
            stack_ld=80, vec=1, hc=1, lds=1, C=2)

VALUES = dict(
    S=[0, -1, 1, 2 ** 31], n=[0, -1, 1, 47, 50, BIG, BIG - 1], T=[0, -1, 1, 2, 3, 4, BIG], f=[0, -1, 1, 3, 8, 40000, 2 ** 30],
    H=[0, -1, 1, 2, 5, 6, 20, 21], N=[0, -1, 1, 7, 32, 33, 2 ** 23, 2 ** 30], K=[0, -1, 1, 2 ** 30],
    bias_kind=[-1, 1, 2, 3], bias_dtype=[-1, 1, 2], as_series=[0], g_as_series=[0], pool=[0, 1, 2, 3, 8, -4],
    stride=[0, -1, 2, 3, 4, 19, 20, 21, 22, BIG], pl=[-1, 1, 2, 3], pr=[-1, 1, 2, 3], dil=[0, -1, 2, 3, 9, 10, BIG],
    ring_ld=[7, 9, 12, 16, BIG, BIG - 1], head=[-1, 1, 2, 3], out_T=[0, -1, 4, 9, 10, 11], out_t0=[-1, 0, 15, 16],
    win_off=[-1, 1, 2], stack_ld=[-1, 0, 1, 8, 2 ** 31 - 1, 2 ** 31], ws=["null", "short", "misaligned"], vec=[0, 2], hc=[0], lds=[0],
    C=[-1, 0, 1, BIG])
VALUES.update({p: [0] for p in POINTERS})
VALUES["bias"] = [1]

# more than one argument moved: the 32-bit bounds, the pads and steps together, one tap, channels the plan refuses
COMBOS = [
    dict(S=1, n=1, T=2 ** 25, f=1), dict(S=1, n=1, T=2 ** 25 - 3, f=1), dict(S=1, n=1, T=2 ** 25, f=1, stack_ld=2 ** 25),
    dict(S=1, n=1, T=2 ** 25 - 3, f=1, stack_ld=2 ** 25), dict(S=1, n=1, T=2 ** 24, f=64, N=1), dict(S=2 ** 20, n=2 ** 20),
    dict(bias=1, bias_kind=1), dict(bias=1, bias_kind=2), dict(bias=1, bias_kind=3), dict(bias=1, bias_kind=1, bias_dtype=1),
    dict(pl=2, pr=0), dict(pl=1, pr=2), dict(pl=2, pr=2, stride=2), dict(pl=2, pr=2, stride=3, f=3), dict(pl=3, pr=3, H=4),
    dict(T=2, pl=1), dict(T=2, pl=2, pr=2), dict(T=1, pl=2, pr=2), dict(stride=24, pl=2, pr=2), dict(stride=25, pl=2, pr=2),
    dict(stride=4, G=0), dict(stride=4, dW=0), dict(stride=2, f=3), dict(stride=2, win_off=1), dict(stride=2, win_off=2), dict(stride=7, win_off=6),
    dict(stride=7, win_off=5), dict(stride=1, win_off=0), dict(stride=1, win_off=1), dict(stride=2, H=1), dict(stride=2, H=1, win_off=1, ring=0),
    dict(stride=2, out=0, win_off=1, T=1), dict(stride=2, pos=0), dict(stride=2, pos=0, head=1), dict(stride=2, pos=0, head=2), dict(stride=2, head=2),
    dict(stride=2, f=40000), dict(stride=2, f=40000, win_off=1, T=1), dict(stride=2, ring_ld=7), dict(stride=2, bias_kind=3),
    dict(dil=2, stride=2), dict(dil=2, pl=2, pr=2), dict(dil=2, pl=4), dict(dil=2, pl=5), dict(dil=2, f=3), dict(dil=2, ring_ld=16),
    dict(dil=2, ring_ld=16, head=3), dict(dil=2, ring_ld=16, head=4), dict(dil=2, ring_ld=15), dict(dil=3, ring_ld=24, T=1),
    dict(H=1, dil=2), dict(H=1, dil=2, stride=2), dict(H=1, dil=0), dict(H=1, ring=0, ring_ld=0), dict(H=1, ring=0, ring_ld=0, dil=2),
    dict(H=1, stack=0), dict(H=1, pos=0), dict(H=1, pool=3),
    dict(pos=0), dict(pos=0, head=1), dict(pos=0, head=2), dict(pos=1, head=2), dict(ring=0, dW=0), dict(ring=0, dW=0, stack=0), dict(ring=0, G=0),
    dict(G=0, dW=0), dict(G=0, W=0), dict(dW=0, stack=0), dict(dW=0, W=0), dict(G=0, stack=0),
    dict(out_T=5, out_t0=0), dict(out_T=5, out_t0=1), dict(out_T=20, out_t0=15, as_series=0), dict(out_T=20, out_t0=16, g_as_series=0),
    dict(f=40000, G=0), dict(f=40000, dW=0), dict(N=40000), dict(N=40000, dW=0), dict(N=40000, G=0), dict(N=2 ** 23, G=0), dict(K=70000, f=1, N=1),
    dict(f=8, stack_ld=88), dict(f=8, stack_ld=84), dict(f=3, stack_ld=64), dict(stack_ld=79), dict(stack_ld=19, T=5), dict(stack_ld=20, T=5),
    dict(ws="short", G=0), dict(ws="short", dW=0), dict(ws="null", stride=2), dict(ws="misaligned", dil=2), dict(ws="short", dil=2, pl=2),
    dict(H=64, f=64, T=64, stack_ld=4096), dict(H=64, f=64, T=64, stack_ld=4096, stride=2), dict(H=8, f=1024), dict(H=8, f=1024, stride=4),
    dict(H=8, f=1021, vec=0), dict(H=3, f=5000, vec=1), dict(H=3, f=5000, vec=0), dict(pool=2, N=64), dict(pool=4, H=1, f=1, N=1),
    dict(hc=0, lds=0), dict(stride=0, pool=3), dict(H=1, f=16000), dict(H=1, f=16500), dict(H=2, f=8000, N=64), dict(H=2, f=3000, N=64, stride=9),
    dict(pos=0, T=0), dict(pos=0, C=-1), dict(T=0, C=-1), dict(T=BIG, C=BIG), dict(T=1, C=0), dict(T=7, C=3), dict(T=-1, C=0), dict(T=0, C=0),
    dict(T=1, C=1), dict(T=2, C=1), dict(T=3, C=7), dict(T=BIG, C=0), dict(T=BIG, C=1), dict(T=1, C=BIG), dict(T=-5, C=-5), dict(pos=0, T=1, C=0),
    dict(H=4, f=2000), dict(H=16, f=256, N=33), dict(H=2, f=2, N=2), dict(H=100, f=100, N=100), dict(H=7, f=7, N=17, vec=0), dict(H=1, f=1, N=1),
    dict(H=5, f=600, stride=2), dict(H=5, f=600, stride=5, pool=2),
    dict(pos=0, T=2, C=2), dict(pos=0, T=-1, C=-1), dict(T=5, C=0), dict(T=5, C=4), dict(T=5, C=5), dict(T=5, C=6), dict(T=9, C=9),
    dict(pos=0, T=BIG, C=BIG), dict(T=4, C=4), dict(T=6, C=2), dict(T=2, C=6), dict(T=16, C=2), dict(T=64, C=62), dict(T=-1, C=-1), dict(T=0, C=BIG),
]


def base_of(name):
    b = dict(BASE)
    if any(tag in name for tag in CHUNKED):
        b.update(T=5, stack_ld=20)
    if "_strided" in name:
        b.update(stride=2)
    return b


def rows_of(name, args):
    """[(label, arguments)]: the base, every argument moved alone, and the combinations that touch only this entry's arguments"""
    b = base_of(name)
    if name in PLANS:
        args = args + ["hc", "lds"]
    moved = [{}] + [{a: v} for a in args if a != "ws_bytes" for v in VALUES.get(a, []) if v != b[a]]
    moved += [c for c in COMBOS if all(k in args for k in c) and any(b[k] != v for k, v in c.items())]
    seen, out = set(), []
    for m in moved:
        label = ",".join("%s=%s" % kv for kv in sorted(m.items())) or "base"
        if label not in seen:
            seen.add(label)
            out.append((label, dict(b, **m)))
    return out


def _ptr(flag, address=16):
    return ctypes.c_void_p(address) if flag else None


def call(L, name, kw):
    """One row's answer: the return code, a query's byte count, or a plan's [rc, hc, lds_bytes]"""
    if name in PLANS:
        hc, lds = ctypes.c_int32(-7), ctypes.c_int32(-7)
        rc = getattr(L, name)(*[kw[a] for a in PLANS[name]], ctypes.byref(hc) if kw["hc"] else None, ctypes.byref(lds) if kw["lds"] else None)
        return [rc, hc.value, lds.value]
    if name in QUERIES:
        return int(getattr(L, name)(*[kw[a] for a in QUERIES[name]]))
    args, query = ENTRIES[name]
    vals = []
    for a in args:
        if a == "ws":
            need = int(getattr(L, query)(*[kw[q] for q in QUERIES[query]]))
            vals.append(None if kw["ws"] == "null" else ctypes.c_void_p(4104 if kw["ws"] == "misaligned" else 4096))
            vals.append(max(need - 1, 0) if kw["ws"] == "short" else need)
        elif a == "ws_bytes":
            continue
        else:
            vals.append(_ptr(kw[a]) if a in POINTERS else kw[a])
    return int(getattr(L, name)(None, *vals))        # the null stream


def table(L):
    """{entry: [[label, answer], ...]} in a fixed order"""
    out = {}
    for name, args in list((k, v[0]) for k, v in ENTRIES.items()) + list(QUERIES.items()) + list(PLANS.items()):
        out[name] = [[label, call(L, name, kw)] for label, kw in rows_of(name, args)]
    return out


def _library():
    import torch
    if torch.cuda.is_available():
        pytest.skip("the table is recorded without a device: an accepted call must fail at its first launch")
    from tgcn_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def answers():
    return table(_library())


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_row_answers_as_the_abi8_library_did(answers, recorded):
    assert sorted(answers) == sorted(recorded)
    for name in recorded:
        assert [r[0] for r in answers[name]] == [r[0] for r in recorded[name]], name
        wrong = [(a[0], a[1], r[1]) for a, r in zip(answers[name], recorded[name]) if a[1] != r[1]]
        assert not wrong, "%s: (row, now, recorded) %s" % (name, wrong[:12])


def test_the_recording_covers_every_answer_an_entry_can_give(recorded):
    """>= 40 rows per entry; an accepted row (-2), a -1, and -4 / -3 wherever the entry has a plan, a grid or a workspace to refuse"""
    assert set(recorded) == set(ENTRIES) | set(QUERIES) | set(PLANS)
    for name, rows in recorded.items():
        assert len(rows) >= 40, (name, len(rows))
        if name in QUERIES:
            assert any(r[1] == 0 for r in rows) and any(r[1] > 0 for r in rows), name
            continue
        codes = {r[1][0] for r in rows} if name in PLANS else {r[1] for r in rows}
        want = {0, -1, -4} if name in PLANS else {-2, -1}
        if name in ENTRIES and name != "tgcn_series_stream_advance":
            want.add(-4)
        if name in ENTRIES and ENTRIES[name][1]:
            want.add(-3)
        assert want <= codes and codes <= want, (name, sorted(codes))
