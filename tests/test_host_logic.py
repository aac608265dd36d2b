"""CPU-only tests of the host side: schedule construction, weight folding, C-ABI surface, error behaviour."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_files, load_golden, rel_err
from oracle import cheb_oracle as O


def _rand_csr(n, m, rng, hubs=()):
    row, col = rng.integers(0, n, m), rng.integers(0, n, m)
    for h, d in hubs:
        row = np.concatenate([row, np.full(d, h)])
        col = np.concatenate([col, rng.integers(0, n, d)])
    val = rng.standard_normal(row.shape[0]).astype(np.float32)
    return row, col, val


@pytest.mark.parametrize("lpr", [1, 4, 16, 64])
def test_schedule_covers_every_entry_once(lpr):
    from tgcn_amd.graph import GraphOperand
    rng = np.random.default_rng(lpr)
    n = 3000
    row, col, val = _rand_csr(n, 20000, rng, hubs=((3, 500), (77, 40), (2999, 9000)))
    op = GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.as_tensor(val))
    s = op.schedule(lpr)
    rowptr = op.rowptr.numpy().astype(np.int64)
    deg = np.diff(rowptr)
    blk = s.blk_row.numpy()
    assert blk[0] == 0 and blk[-1] == n and np.all(np.diff(blk) >= 0) and len(blk) == s.nblk + 1
    covered = np.zeros(op.nnz, np.int32)
    for r in np.nonzero(deg <= s.row_thresh)[0]:
        covered[rowptr[r]:rowptr[r + 1]] += 1
    seg_row, e0, e1, slot = (t.numpy() for t in (s.seg_row, s.seg_e0, s.seg_e1, s.seg_slot))
    wave_max = 128 if lpr == 16 else 0          # whole-row wave segments: 16-lane schedules only
    assert s.nwseg == int(((deg > s.row_thresh) & (deg <= wave_max)).sum())          # medium rows: one whole-row wave segment each
    for i in range(s.nseg):
        assert rowptr[seg_row[i]] <= e0[i] < e1[i] <= rowptr[seg_row[i] + 1]
        if i < s.nwseg:
            assert e0[i] == rowptr[seg_row[i]] and e1[i] == rowptr[seg_row[i] + 1] and s.row_thresh < e1[i] - e0[i] <= wave_max and slot[i] < 0
        else:
            assert e1[i] - e0[i] <= s.seg_len and deg[seg_row[i]] > max(wave_max, s.row_thresh)
        covered[e0[i]:e1[i]] += 1
        whole = (e0[i] == rowptr[seg_row[i]] and e1[i] == rowptr[seg_row[i] + 1])
        assert (slot[i] < 0) == whole
    assert np.all(covered == 1)
    # slots of a long row are consecutive and in column (entry) order; every slot is used exactly once
    long_row, long_slot = s.long_row.numpy(), s.long_slot.numpy()
    assert long_slot[0] == 0 and long_slot[s.nlong] == s.npartial
    used = np.sort(slot[slot >= 0])
    assert np.array_equal(used, np.arange(s.npartial))
    for i in range(s.nlong):
        mine = np.nonzero(seg_row == long_row[i])[0]
        mine = mine[np.argsort(e0[mine])]
        assert np.array_equal(slot[mine], np.arange(long_slot[i], long_slot[i + 1]))
    nslots = np.diff(long_slot[: s.nlong + 1])
    assert np.all(nslots[: s.nhuge] > 64) and np.all(nslots[s.nhuge:] <= 64)
    # wave rows and lane-group segments are each stored in order of their first column
    first_col = op.edges[:, 0].numpy()[e0[: s.nseg]]
    assert np.all(np.diff(first_col[: s.nwseg]) >= 0) and np.all(np.diff(first_col[s.nwseg:]) >= 0)


def test_dense_copy_of_small_dense_operands():
    """Operands with n <= 256 that store >= 1/4 of their entries carry a dense copy (duplicates summed) for the
    matrix-pipe kernels; sparse or larger ones do not."""
    from tgcn_amd.graph import GraphOperand
    rng = np.random.default_rng(5)
    n = 40
    row, col = rng.integers(0, n, 900), rng.integers(0, n, 900)            # with duplicates
    val = rng.standard_normal(900).astype(np.float32)
    op = GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.as_tensor(val))
    assert op.dense is not None and op.struct.dense == op.dense.data_ptr()
    ref = np.zeros((n, n), np.float64)
    np.add.at(ref, (row, col), val.astype(np.float64))
    assert np.abs(op.dense.numpy() - ref).max() <= 1e-5
    sparse = GraphOperand.from_coo(n, torch.as_tensor(row[:100]), torch.as_tensor(col[:100]), torch.as_tensor(val[:100]))
    assert sparse.dense is None and not sparse.struct.dense
    big = GraphOperand.from_coo(300, torch.as_tensor(rng.integers(0, 300, 40000)), torch.as_tensor(rng.integers(0, 300, 40000)),
                                torch.as_tensor(rng.standard_normal(40000).astype(np.float32)))
    assert big.dense is None


def test_operand_constructors_agree():
    from tgcn_amd.graph import GraphOperand
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    n = 50
    D = (rng.random((n, n)) < 0.1) * rng.standard_normal((n, n))
    D = D.astype(np.float32)
    ref = sp.csr_matrix(D)
    for L in (torch.tensor(D), torch.tensor(D).to_sparse(), torch.tensor(D).to_sparse_csr(), ref, D):
        op = GraphOperand.from_any(L, "cpu")
        assert (op.to_scipy() != ref).nnz == 0
    t = GraphOperand.from_any(ref, "cpu").transpose().to_scipy()
    assert (t != ref.T.tocsr()).nnz == 0


def test_edge_operand_matches_oracle():
    from tgcn_amd.graph import GraphOperand
    g = load_golden([f for f in golden_files("ChebConv_") if "rmat1024" in f][0])
    n = int(g["n"])
    op = GraphOperand.from_edge_index(torch.as_tensor(g["edge_index"]), torch.as_tensor(g["edge_weight"]), n)
    row, col, lap = O.edge_laplacian(g["edge_index"], g["edge_weight"], n)
    ref = O.coo_to_csr(row, col, lap, n)
    assert abs(op.to_scipy() - ref).max() <= 1e-7


@pytest.mark.parametrize("K", [1, 2, 3, 5, 10, 25])
def test_power_fold_is_the_reference_recursion(K):
    """sum_k Xt[k] W[k] (reference_power stack) == sum_j (L^j x) W'[j] with W' = fold(W)."""
    from tgcn_amd.functional import power_fold_matrix
    g = load_golden([f for f in golden_files("GCNCheb_") if "dti148" in f][0])
    L = O.csr_from_arrays(g["n"], g["rowptr"], g["col"], g["val"]).astype(np.float64)
    rng = np.random.default_rng(K)
    x = rng.standard_normal((2, int(g["n"]), 3))
    W = rng.standard_normal((K, 3, 4))
    ref = np.einsum("kqnf,kfg->qng", O.stack_reference_power(L, x, K), W)
    c = power_fold_matrix(K, dtype=torch.float64).numpy()
    Wf = np.einsum("kj,kfg->jfg", c, W)
    P = [x]
    for _ in range(1, K):
        P.append(O._apply(L, P[-1]))
    got = np.einsum("kqnf,kfg->qng", np.stack(P), Wf)
    assert rel_err(got, ref) <= 1e-12


def test_c_abi_exports_every_declared_symbol():
    from tgcn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tgcn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(tgcn_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert _lib.lib().tgcn_abi_version() == _lib.ABI_VERSION == 8


def _kernel_resources():
    """{demangled-ish kernel name: {vgpr_count, sgpr_count, spills}} read from the code object inside the built library (llvm-objcopy +
    clang-offload-bundler + llvm-readelf of the ROCm toolchain: under a second, no recompilation)"""
    import subprocess
    import tempfile
    from tgcn_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not all(os.path.exists(os.path.join(llvm, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.elf")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", _lib.LIB_PATH, fat], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = dict(vgpr=int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)), sgpr=int(re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1)),
                         spill=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    return out


def test_hot_kernels_keep_their_register_budget():
    """Occupancy is part of the design: the row-mapped bf16x3 projection runs TWO 512-thread workgroups per CU (<= 128
    VGPRs) and the hop kernels seven or eight 256-thread workgroups.  Round 4 lost the first silently once -- two 64-bit divisions in a shared
    row-map helper took project_x3_kernel<4, true> from 124 to 138 registers and the projection of the headline from 44 to 67 ms -- so the
    budgets are asserted on the binary that ships."""
    res = _kernel_resources()

    def find(*parts):
        hits = [v for k, v in res.items() if all(p in k for p in parts)]
        assert len(hits) == 1, (parts, [k for k in res if parts[0] in k][:5])
        return hits[0]
    x3 = find("project_x3_kernelILi4ELb1")                      # cfg5's projection (N = 64, aligned rows)
    assert x3["vgpr"] <= 128 and x3["spill"] == 0, x3
    hop = find("hop_kernelILi16ELi4ELi8ELi1ELi7")                # cfg5's hop: 16-lane groups, 8 gathers in flight, streaming hints
    assert hop["vgpr"] <= 72 and hop["spill"] == 0, hop          # 7 waves per SIMD
    assert find("hop_kernelILi4ELi4ELi4ELi1ELi0")["vgpr"] <= 64  # cfg5n's hop: 8 waves per SIMD
    assert find("project_narrow_kernel")["vgpr"] <= 128
    # round 5: the streaming bf16x3 projection runs ONE 1024-thread workgroup per CU = 4 waves per SIMD: 128 VGPRs, nothing spilled
    for nt in (1, 2, 4):
        for kt in (1, 2):
            st = find("project_x3_stream_kernelILi%dELi%dE" % (nt, kt))
            assert st["vgpr"] <= 128 and st["spill"] <= 8, (nt, kt, st)


def test_geometry_queries():
    from tgcn_amd import _lib
    L = _lib.lib()
    assert (L.tgcn_hop_vec_width(64, 1), L.tgcn_hop_lanes_per_row(64, 1)) == (4, 16)
    assert (L.tgcn_hop_vec_width(64, 0), L.tgcn_hop_lanes_per_row(64, 0)) == (1, 64)
    assert (L.tgcn_hop_vec_width(28, 1), L.tgcn_hop_lanes_per_row(28, 1)) == (4, 8)
    assert (L.tgcn_hop_vec_width(1, 1), L.tgcn_hop_lanes_per_row(1, 1)) == (1, 1)
    assert L.tgcn_hop_lanes_per_row(1200, 1) == 64 and L.tgcn_hop_groups_per_block(1200, 1) == 4


def test_bad_arguments_return_error_codes_not_crashes():
    from tgcn_amd import _lib
    L = _lib.lib()
    assert L.tgcn_csr_hop_f32(None, None, None, 1, 4, None, None, 1.0, 0.0, None, None, None, 0) == -1
    assert b"null" in L.tgcn_last_error()
    assert L.tgcn_relayout_qnc_to_nqc_f32(None, None, None, 1, 1, 1) == -1
    assert L.tgcn_pool_max_f32(None, None, None, None, 1, 3, 1, 2) == -1
    assert L.tgcn_set_tuning(b"nope", 1) == -1
    for retired in (b"fuse_last_hop", b"compact_proj", b"overlap"):      # removed with ABI v8: unknown keys like any other
        assert L.tgcn_set_tuning(retired, 1) == -1 and b"unknown key" in L.tgcn_last_error()


def test_operand_rejects_out_of_range_indices():
    from tgcn_amd.graph import GraphOperand
    from tgcn_amd._lib import TgcnError
    with pytest.raises(TgcnError):
        GraphOperand.from_coo(4, torch.tensor([0, 1]), torch.tensor([1, 4]), torch.tensor([1.0, 1.0]))
    with pytest.raises(TgcnError):
        GraphOperand.from_coo(4, torch.tensor([0, -1]), torch.tensor([1, 2]), torch.tensor([1.0, 1.0]))
    with pytest.raises(TgcnError):
        GraphOperand.from_edge_index(torch.tensor([[0, 1], [1, 7]]), None, 4)


def test_modules_refuse_cpu_tensors():
    import tgcn_amd
    from tgcn_amd._lib import TgcnError
    layer = tgcn_amd.GCNCheb(torch.eye(4), 1, 2, 2)
    with pytest.raises(TgcnError):
        layer(torch.randn(2, 4))
    with pytest.raises(TgcnError):
        tgcn_amd.gcn_pool(torch.randn(1, 4, 2))
    conv = tgcn_amd.ChebConv(1, 2, 3)
    with pytest.raises(TgcnError):
        conv(torch.randn(2, 4), torch.tensor([[0, 1], [1, 0]]))


def test_module_surface_matches_reference():
    """Parameter names / shapes / init bound / repr, as the reference's state_dict and scripts expect
    (tgcn/nn/gcn.py:10-31, 84-105, 160-181, 377-394, 474-491)."""
    import tgcn_amd
    L = torch.eye(6)
    m = tgcn_amd.TGCNCheb(L, 3, 5, 4)
    assert m.weight.shape == (4, 3, 5) and m.bias.shape == (1, 6, 5) and list(m.state_dict()) == ["weight", "bias"]
    m = tgcn_amd.TGCNCheb_H(L, 1, 5, 4, 7)
    assert m.weight.shape == (4, 7, 1, 5) and m.bias.shape == (1, 6, 5)
    m = tgcn_amd.GCNCheb(L, 3, 5, 4, bias=False)
    assert m.weight.shape == (4, 3, 5) and m.bias is None and list(m.state_dict()) == ["weight"]
    assert repr(m) == "GCNCheb(3, 5, filter_order=4)"
    m = tgcn_amd.ChebConv(3, 5, 4)
    assert m.weight.shape == (4, 3, 5) and m.bias.shape == (5,) and repr(m) == "ChebConv(3, 5, K=4)"
    m = tgcn_amd.ChebTimeConv(2, 5, 4, 7)
    assert m.weight.shape == (4, 7, 2, 5) and m.bias.shape == (5,)
    bound = 1.0 / np.sqrt(2 * 4)
    assert m.weight.abs().max() <= bound and m.bias.abs().max() <= bound
    g = load_golden(golden_files("uniform_pool")[0])
    torch.manual_seed(int(g["uniform_seed"]))
    t = torch.empty(7, 5, 3)
    tgcn_amd.uniform(int(g["uniform_size"]), t)
    assert np.array_equal(t.numpy(), g["uniform_out"])        # same RNG stream as the reference's uniform()


def test_compat_import_paths():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "from tgcn.nn.gcn import TGCNCheb, TGCNCheb_H, GCNCheb, ChebConv, ChebTimeConv, gcn_pool, gcn_pool_4, uniform, spmm, spmm_batch_2, spmm_batch_3;"
            "from tgcn.nn.gcn_matmul import GCNCheb as G2; from gcn.graph import chebyshev; import tgcn_amd; assert G2 is tgcn_amd.GCNCheb"
            % (ROOT, os.path.join(ROOT, "compat")))
    subprocess.run([sys.executable, "-c", code], check=True)


# A stand-in for a reference checkout behind compat/: a `gcn` package whose graph.py defines the helpers the shim delegates (written for
# this test; small numpy / scipy versions of the same functions, not the reference's code).  The delegation under test does not care whose
# graph.py it finds, only that it is the file behind compat/ on sys.path.
_STANDIN_GRAPH = """
import numpy as np
import scipy.sparse
import scipy.sparse.linalg
import scipy.spatial.distance


def grid(m, dtype=np.float32):
    xx, yy = np.meshgrid(np.linspace(0, 1, m, dtype=dtype), np.linspace(0, 1, m, dtype=dtype))
    return np.stack([xx.ravel(), yy.ravel()], axis=1)


def distance_scipy_spatial(z, k=4, metric="euclidean"):
    d = scipy.spatial.distance.squareform(scipy.spatial.distance.pdist(z, metric))
    idx = np.argsort(d, axis=1)[:, 1:k + 1]
    return np.take_along_axis(d, idx, axis=1), idx


def distance_sklearn_metrics(z, k=4, metric="euclidean"):
    return distance_scipy_spatial(z, k, metric)


def adjacency(dist, idx):
    n, k = dist.shape
    sigma2 = np.mean(dist[:, -1]) ** 2
    w = np.exp(-dist ** 2 / sigma2)
    W = scipy.sparse.coo_matrix((w.ravel(), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n)).tocsr()
    W.setdiag(0)
    return W.maximum(W.T)


def laplacian(W, normalized=True):
    d = np.asarray(W.sum(axis=0)).ravel()
    if not normalized:
        return scipy.sparse.diags(d) - W
    s = 1 / np.sqrt(d + np.spacing(1))
    D = scipy.sparse.diags(s)
    return scipy.sparse.identity(W.shape[0], dtype=W.dtype) - D @ W @ D


def lmax(L, normalized=True):
    return 2.0 if normalized else float(scipy.sparse.linalg.eigsh(L, k=1, which="LM", return_eigenvectors=False)[0])


def rescale_L(L, lmax=2):
    return (2.0 / lmax) * L - scipy.sparse.identity(L.shape[0], dtype=L.dtype)


def fourier(L):
    return np.linalg.eigh(L.toarray())


def lanczos(L, X, K):
    raise NotImplementedError


def replace_random_edges(A, noise_level):
    return A


def chebyshev(L, X, K):
    raise NotImplementedError
"""


def _standin_reference(root):
    """<root>/gcn/{__init__,graph}.py: what the shim looks for behind compat/ on sys.path"""
    pkg = root / "gcn"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    (pkg / "graph.py").write_text(_STANDIN_GRAPH)
    return str(root)


def _run_with_path(code, cwd, *entries):
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(entries), PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run([sys.executable, "-c", code], env=env, cwd=str(cwd), capture_output=True, text=True)


def test_compat_gcn_graph_delegates_to_the_reference(tmp_path):
    """With PYTHONPATH=compat:repo:reference `import gcn.graph as graph` serves chebyshev from this repo and every
    other name from the checkout's own gcn/graph.py, so examples/tgcn_mnist.py:52-54,173-175,194 and
    examples/pytorch_based/pytorch_hcp_tgcn.py:13,52-57 run unchanged; nothing of the reference is copied or imported under its public name.
    The checkout is a stand-in written under tmp_path (_STANDIN_GRAPH), so the test needs nothing outside the repository."""
    reference = _standin_reference(tmp_path / "reference")
    work = tmp_path / "cwd"
    work.mkdir()
    code = """
import sys
import numpy as np
import gcn.graph as graph, gcn.coarsening as coarsening
import tgcn_amd.numpy_api, tgcn_amd.coarsening
assert graph.chebyshev is tgcn_amd.numpy_api.chebyshev
assert coarsening.coarsen is tgcn_amd.coarsening.coarsen and coarsening.perm_data is tgcn_amd.coarsening.perm_data
ref = sys.modules.get("gcn._reference_graph")
assert ref is None                                     # loaded lazily, on the first delegated name
z = graph.grid(4)                                      # examples/tgcn_mnist.py:173
ref = sys.modules["gcn._reference_graph"]
assert ref.__file__ == %r and graph.grid is ref.grid
dist, idx = graph.distance_sklearn_metrics(z, k=4, metric="euclidean")   # :174
A = graph.adjacency(dist, idx)                         # :175
L = graph.rescale_L(graph.laplacian(A, normalized=True), lmax=2)          # :194, :54
assert L.shape == (16, 16) and abs(L.diagonal()).max() < 1e-6
for name in ("fourier", "lanczos", "lmax", "replace_random_edges", "distance_scipy_spatial"):
    assert getattr(graph, name) is getattr(ref, name)
assert "grid" in dir(graph) and "chebyshev" in dir(graph)
assert ref.chebyshev is not graph.chebyshev            # the reference's own twin stays reachable only under the private name
try:
    graph.no_such_function
except AttributeError as e:
    assert "no_such_function" in str(e)
else:
    raise AssertionError("missing name must raise AttributeError")
import gcn
assert any(p.startswith(%r) for p in gcn.__path__)      # gcn.models / gcn.utils resolve to the reference's files
print("ok")
""" % (os.path.join(reference, "gcn", "graph.py"), reference)
    r = _run_with_path(code, work, os.path.join(ROOT, "compat"), ROOT, reference)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_compat_gcn_graph_without_a_reference_checkout_says_so(tmp_path):
    """Only chebyshev is native; asking for a delegated name without a checkout behind compat/ is an AttributeError naming the cause (so that
    attribute probes -- hasattr, getattr with a default, pickle.whichmodule -- see a miss), and an ImportError for `from gcn.graph import name`."""
    code = """
import gcn.graph as graph
assert callable(graph.chebyshev)
assert not hasattr(graph, "grid") and getattr(graph, "rescale_L", None) is None
try:
    graph.grid(4)
except AttributeError as e:
    assert "checkout" in str(e) and "gcn/graph.py" in str(e), str(e)
    assert type(e.__cause__).__name__ == "ReferenceNotFound"
else:
    raise SystemExit("no error")
try:
    from gcn.graph import laplacian
except ImportError as e:
    assert "laplacian" in str(e)
else:
    raise SystemExit("no import error")
import pickle, sys
assert pickle.whichmodule(len, "len") == "builtins"        # scans sys.modules with getattr(module, name, None): must not blow up on the shim
print("ok")
"""
    r = _run_with_path(code, tmp_path, os.path.join(ROOT, "compat"), ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_modules_survive_deepcopy_and_pickle():
    """copy.deepcopy(model) (best-model snapshots, EMA) and torch.save(model) must not trip over the operand cache."""
    import copy
    import io
    import pickle
    import tgcn_amd
    L = torch.eye(12)
    layer = tgcn_amd.TGCNCheb_H(L, 1, 4, 3, 5)
    layer._ops.get(("k",), lambda: object(), sources=(L,))          # something unpicklable-ish in the cache
    twin = copy.deepcopy(layer)
    assert torch.equal(twin.weight, layer.weight) and twin._ops._d == {}
    buf = io.BytesIO()
    pickle.dump(layer, buf)
    back = pickle.loads(buf.getvalue())
    assert torch.equal(back.weight, layer.weight) and back._ops._d == {}
    conv = copy.deepcopy(tgcn_amd.ChebConv(2, 3, 4))
    assert conv.weight.shape == (4, 2, 3)


def test_operand_cache_evicts_least_recently_used_only():
    """past 16 entries the cache used to drop everything; a training loop that swaps edge_index per subject
    (examples/pytorch_geo_based/pygeo_hcp.py:284) must keep the operands it keeps coming back to."""
    from tgcn_amd.nn import _OperandCache
    cache = _OperandCache()
    built = []
    mk = lambda k: (lambda: built.append(k) or ("op", k))
    for k in range(16):
        cache.get(k, mk(k))
    assert cache.get(0, mk(0)) == ("op", 0) and built == list(range(16))      # hit: entry 0 is now the most recent
    cache.get(16, mk(16))                                                     # evicts entry 1, the least recently used
    assert len(cache._d) == 16 and 0 in cache._d and 1 not in cache._d and 16 in cache._d
    cache.get(1, mk(1))
    assert built == list(range(17)) + [1] and 2 not in cache._d


def test_scipy_and_ndarray_operands_are_keyed_by_their_whole_content():
    """a scipy / ndarray L has no version counter; the cache key is a hash of ALL of data (+ indices, indptr), so an
    in-place edit anywhere -- gcn/graph.py:236 rescales L.data in place for lmax != 2, examples/gcn_mnist.py:131 rebuilds L between calls --
    is a new key.  (Round 5 tagged the first and last 32 values only.)  The numpy_api cache is LRU and locked like the modules' own."""
    import threading
    import scipy.sparse as sp
    from tgcn_amd import numpy_api
    from tgcn_amd.nn import _np_fingerprint
    rng = np.random.default_rng(3)
    L = sp.random(400, 400, 0.05, format="csr", dtype=np.float32, random_state=3)
    assert L.nnz > 200
    base = _np_fingerprint(L)
    assert base == _np_fingerprint(L) == numpy_api._fingerprint(L)
    L.data[L.nnz // 2] *= 1.5                                   # an edit in the MIDDLE of the stored values
    mid = _np_fingerprint(L)
    assert mid != base
    L.indices[L.nnz // 2], L.indices[L.nnz // 2 - 1] = L.indices[L.nnz // 2 - 1], L.indices[L.nnz // 2]      # the pattern counts too
    assert _np_fingerprint(L) != mid
    for fmt in ("coo", "csc"):
        M = L.asformat(fmt)
        a = _np_fingerprint(M)
        M.data[M.nnz // 3] += 1.0
        assert _np_fingerprint(M) != a
    D = rng.standard_normal((50, 50))
    a = _np_fingerprint(D)
    D[25, 25] += 1.0
    assert _np_fingerprint(D) != a
    # LRU + lock
    cache = numpy_api._LruCache(max_entries=3)
    built = []
    for k in range(3):
        cache.get(k, lambda k=k: built.append(k) or k)
    cache.get(0, lambda: built.append("again"))                 # hit: most recent
    cache.get(3, lambda: built.append(3) or 3)                  # evicts 1 only
    assert built == [0, 1, 2, 3] and list(cache._d) == [2, 0, 3]
    barrier, got = threading.Barrier(6), [None] * 6

    def worker(i):
        barrier.wait()
        got[i] = cache.get("shared", object)
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(6)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert all(g is got[0] for g in got)


def test_learnable_operand_values_are_never_silently_ignored():
    """Reference: lap = -deg[row] * edge_weight * deg[col] and spmm's `value` are differentiable (tgcn/nn/gcn.py:413,510,296-308).  The MODULES
    and spmm* carry that gradient (tests/test_values_grad.py, GPU); the low-level operand builder, which packs values outside autograd,
    refuses a weight that requires grad instead of dropping its gradient."""
    import tgcn_amd
    from tgcn_amd import _lib
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    w = torch.ones(3, requires_grad=True)
    with pytest.raises(_lib.TgcnError, match="requires_grad"):
        tgcn_amd.GraphOperand.from_edge_index(ei, w, 3)
    assert tgcn_amd.GraphOperand.from_edge_index(ei, w.detach(), 3).nnz == 3      # detached weights build (CPU tensors: the torch form)
    with pytest.raises(_lib.TgcnError, match="ROCm device"):                       # no CPU fallback for the differentiable ops either
        tgcn_amd.spmm(ei, w, 3, torch.ones(3, 2))


def test_operand_cache_is_thread_safe():
    """nn.DataParallel runs replica forwards in threads that share the module's operand cache (and the fold-matrix cache):
    concurrent first uses must build each entry once and hand every thread the same object."""
    import threading
    from tgcn_amd import functional as F
    from tgcn_amd.nn import _OperandCache
    cache = _OperandCache()
    built = []
    barrier = threading.Barrier(8)
    got = [None] * 8

    def build():
        built.append(1)
        import time
        time.sleep(0.01)
        return object()

    def worker(i):
        barrier.wait()
        got[i] = cache.get(("k", i % 2), build)
        F.power_fold_matrix(7 + i % 2, "cpu")

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(built) == 2
    assert all(got[i] is got[i % 2] for i in range(8))


@pytest.mark.parametrize("symmetric", [True, False])
def test_compact_plan_arrays(symmetric, monkeypatch):
    """graph.CompactPlan on CPU tensors: the non-empty rows in order, both operands over the same rows and entry order, columns of
    `rest` in compact ids with entries into empty rows pointing at the zero row -- so that rest @ P (P: compact rows + a zero row)
    equals the rows of L @ P_full for every P_full that is zero on the empty rows (what hop tensors are for k >= 1)."""
    from tgcn_amd import graph
    monkeypatch.setattr(graph, "COMPACT_MIN_ROWS", 1)
    rng = np.random.default_rng(7)
    n = 500
    keep = rng.random(n) < 0.5
    src = rng.integers(0, n, 4000)
    dst = rng.integers(0, n, 4000)
    if symmetric:
        ok = keep[src] & keep[dst]
        row, col = np.concatenate([src[ok], dst[ok]]), np.concatenate([dst[ok], src[ok]])
    else:
        ok = keep[src]
        row, col = src[ok], dst[ok]                 # columns may be vertices without entries of their own
    val = rng.standard_normal(row.shape[0]).astype(np.float32)
    op = graph.GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.as_tensor(val))
    plan = op.compact_plan()
    deg = np.bincount(row, minlength=n)
    assert plan is not None and op.compact_plan() is plan           # built once
    rows, empty = plan.rows.numpy(), plan.empty.numpy()
    assert np.array_equal(rows, np.flatnonzero(deg > 0)) and np.array_equal(empty, np.flatnonzero(deg == 0))
    assert plan.n_c == len(rows) and plan.n_empty == len(empty) and plan.first.n == plan.rest.n == plan.n_c
    assert plan.first.n_cols == n and plan.rest.n_cols == plan.n_c + 1 and plan.first.nnz == plan.rest.nnz == op.nnz
    assert plan.first.edges.data_ptr() == op.edges.data_ptr()       # hop 1 shares the operand's entry array
    assert torch.equal(plan.first.rowptr, plan.rest.rowptr) and plan.first._sched is plan.rest._sched
    L = op.to_scipy().astype(np.float64)
    P_full = rng.standard_normal((n, 3))
    P_full[empty] = 0
    cid = np.full(n, plan.n_c)
    cid[rows] = np.arange(plan.n_c)
    e = plan.rest.edges.numpy()[: op.nnz]
    assert np.array_equal(e[:, 0], cid[op.edges.numpy()[: op.nnz, 0]])
    if not symmetric:
        assert (e[:, 0] == plan.n_c).any()
    import scipy.sparse as sp
    rp = plan.rest.rowptr.numpy()
    rest = sp.csr_matrix((e[:, 1].copy().view(np.float32).astype(np.float64), e[:, 0], rp), shape=(plan.n_c, plan.n_c + 1))
    P_c = np.concatenate([P_full[rows], np.zeros((1, 3))])
    assert np.allclose(rest @ P_c, (L @ P_full)[rows])
    first = sp.csr_matrix((e[:, 1].copy().view(np.float32).astype(np.float64), op.edges.numpy()[: op.nnz, 0], rp), shape=(plan.n_c, n))
    x = rng.standard_normal((n, 3))
    assert np.allclose(first @ x, (L @ x)[rows])
    # operands without (enough) empty rows, or below the size threshold, decline
    monkeypatch.setattr(graph, "COMPACT_MIN_ROWS", 1 << 16)
    op2 = graph.GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.as_tensor(val))
    assert op2.compact_plan() is None


@pytest.mark.parametrize("lpr", [4, 16])
def test_wave_segment_schedule_shapes(lpr, monkeypatch):
    """seg_mode 1 (one wave per segment): segments of 32 * (64 / lanes) entries, rows up to that length are whole-row segments"""
    from tgcn_amd import graph
    monkeypatch.setattr(graph, "SEG_MODE", 1)
    rng = np.random.default_rng(lpr)
    n = 2000
    wave_len = 32 * (64 // lpr)
    row, col, val = _rand_csr(n, 9000, rng, hubs=((3, wave_len), (77, wave_len + 1), (500, 5 * wave_len + 3), (1999, 33)))
    op = graph.GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.as_tensor(val))
    s = op.schedule(lpr)
    assert s.seg_mode == 1 and s.seg_len == wave_len and s.struct.seg_mode == 1
    rowptr = op.rowptr.numpy().astype(np.int64)
    deg = np.diff(rowptr)
    seg_row, e0, e1, slot = (t.numpy()[: s.nseg] for t in (s.seg_row, s.seg_e0, s.seg_e1, s.seg_slot))
    assert np.all(e1 - e0 <= wave_len)
    for r in np.flatnonzero(deg > s.row_thresh):
        mine = np.flatnonzero(seg_row == r)
        assert len(mine) == -(-deg[r] // wave_len)
        assert (slot[mine] < 0).all() == (deg[r] <= wave_len)
    assert s.nlong == int((deg > wave_len).sum())
    assert graph.Schedule(op.rowptr, n, 64, edges=op.edges).seg_mode == 0      # a whole wave per row chunk: nothing to fold


def test_hub_first_reordering_warns_and_spreads_the_hot_block():
    """a hub-first order is a pessimisation on power-law graphs (measured, profiles/r05_exp_reorder_degree.log), so
    asking for one says so; the hot block of the order is bit-reversed (neighbours in popularity are not neighbours in the sweep)."""
    import warnings
    from tgcn_amd.graph import GraphOperand, _spread_hot_block
    rng = np.random.default_rng(2)
    n = 4096
    row = np.minimum((rng.random(40000) ** 3 * n).astype(np.int64), n - 1)
    col = rng.integers(0, n, 40000)
    op = GraphOperand.from_coo(n, torch.as_tensor(row), torch.as_tensor(col), torch.ones(40000))
    with pytest.warns(UserWarning, match="hub-first vertex order is measured"):
        a = op.reordered("hub_first")
    with pytest.warns(UserWarning, match="renamed 'hub_first'"):
        b = op.reordered("degree")
    with pytest.warns(UserWarning, match="hub-first"):
        c = op.reordered("degree_sorted")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        op.reordered("rcm")
    assert torch.equal(a.perm, b.perm) and torch.equal(torch.sort(a.perm)[0], torch.arange(n))
    deg = (op.rowptr[1:] - op.rowptr[:-1]).long()
    assert torch.equal(c.perm, torch.argsort(deg, descending=True, stable=True))
    live = int((deg > 0).sum())
    H = 1 << ((live // 8).bit_length() - 1)
    assert 16 <= H < n and torch.equal(a.perm[H:], c.perm[H:]) and not torch.equal(a.perm[:H], c.perm[:H])
    assert torch.equal(torch.sort(a.perm[:H])[0], torch.sort(c.perm[:H])[0])
    assert torch.equal(_spread_hot_block(torch.arange(16), 64), torch.tensor([0, 4, 2, 6, 1, 5, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15]))
    with pytest.raises(Exception, match="unknown order"):
        op.reordered("random")


def test_hot_kernels_do_not_spill():
    """project_x3_stream_kernel runs 1024-thread workgroups at exactly 128 VGPRs with up to 150 KB of dynamic LDS; a compiler update
    that makes it (or the hop kernel) spill would show up only as a slower bench.  The gfx950 code object's own metadata says what the BUILT
    library uses (tools/kernel_resources.py): the hop kernel of the headline and the wide bf16x3 projection must be spill-free, the streaming
    projection may keep the ONE loop-invariant 64-bit address it parks in scratch across its weight-staging prologue today (<4, 2>: 2 VGPRs,
    12 bytes, stored and loaded once per wave, outside the tile loop; round 5's binary parked four) and nothing more."""
    import shutil
    from tgcn_amd import _lib
    from tools import kernel_resources as kr
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("needs the built library and llvm-readelf")
    import hashlib
    before = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    res = kr.kernel_resources(_lib.LIB_PATH)
    assert hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest() == before      # reading the metadata must not rewrite the product library
    assert len(res) > 200
    by = lambda frag: {k: v for k, v in res.items() if frag in k}          # noqa: E731 -- mangled names
    hop = by("10hop_kernelILi16ELi4ELi8ELi1E")
    stream = by("24project_x3_stream_kernel")
    wide = by("19project_x3v2_kernel")
    assert len(hop) >= 4 and len(stream) == 6 and len(wide) >= 5
    for name, r in list(hop.items()) + list(wide.items()):
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    for name, r in stream.items():
        assert r["vgpr_count"] <= 128, (name, r)                              # 1024 threads per workgroup: 4 waves per SIMD
        assert r["vgpr_spill_count"] <= 2 and r["private_segment_fixed_size"] <= 12 and r["uses_dynamic_stack"] in ("false", 0), (name, r)
    assert shutil.which("true")
