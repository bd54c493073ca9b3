"""CPU suite, part 3: the N > 1 path over `gloo` with world_size 2 (and 3).

No GPU exists here, so each rank's LOCAL product is executed by the packed-image interpreter of
tests/_common.py (the same image the HIP kernel walks); everything else -- the block-row partition,
the ownership ranges handed to the C ABI, the point-to-point halo reduce of the symmetric path and
the y all-gather -- is the real code of blocksparsematrices.jl_amd/distributed.py.
The rank process is tests/_distworker.py, shared with tests/test_fuzz_distributed_cpu.py.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _distworker import free_port as _free_port  # noqa: E402
from _distworker import spawn  # noqa: E402


@pytest.mark.parametrize("kind,world", [("vbcrs", 2), ("symmetric", 2), ("symmetric", 3), ("blocksparse", 2),
                                        ("blocksparse", 3), ("vbcrs_T_across", 2), ("vbcrs_cols_T", 2),
                                        ("vbcrs_tiny", 3)])
def test_row_partitioned_over_gloo(kind, world):
    """the rank process is tests/_distworker.py (shared with the fuzz tests)"""
    status, errs, own, touched, codes = spawn(kind, world)
    assert status == "ok", errs
    assert all(e < 1e-12 for e in errs), " ".join("%.2e" % e for e in errs)
    assert all(c == 0 for c in codes)


@pytest.mark.parametrize("touched", [(1, 40), (1, 48)])  # no halo: straight into y; a halo: through the work matrix
def test_local_product_gets_vectors_from_mul_and_matrices_from_mul_multi(monkeypatch, touched):
    """mul and mul_multi share one body on (n, K) views; the local product of mul must still see vectors (bsm_mul), not
    (n, 1) matrices (the one-column bsm_mul_multi)"""
    sys.path.insert(0, ROOT)
    from bsm_amd import distributed as D
    dims = []
    monkeypatch.setattr(D.M, "mul", lambda yy, A, xx, a, b: dims.append((yy.dim(), xx.dim())) or yy)
    P = D.RowPartitioned(object(), (1, 40), touched)
    y, x = torch.zeros(48, dtype=torch.float64), torch.ones(48, dtype=torch.float64)
    P.mul(y, x)
    P.mul(y, x, 0.5, -2.0, x_distributed=True)
    P.mul_multi(torch.zeros((3, 48), dtype=torch.float64).t(), torch.ones((3, 48), dtype=torch.float64).t())
    assert dims == [(1, 1), (1, 1), (2, 2)]


def test_partition_is_a_partition():
    sys.path.insert(0, ROOT)
    import bsm_amd as bsm
    from bsm_amd import distributed as D
    prob = bsm.synthetic.config2(n=8000, nblocks=500)
    seen, prev_hi = 0, 0
    for r in range(4):
        local, own = D.split_vbcrs(prob, r, 4)
        seen += len(local["blocks"])
        assert own[0] == prev_hi + 1
        prev_hi = own[1]
        for rs, b in zip(local["rowstart"], local["blocks"]):
            assert own[0] <= rs and rs + b.shape[0] - 1 <= own[1]
    assert seen == len(prob["blocks"]) and prev_hi == 8000
    sp = bsm.synthetic.config3(nseg=30, bs=16, halfband=4)
    nd = no = 0
    for r in range(3):
        local, own, touched = D.split_symmetric(sp, r, 3)
        nd += len(local["diagonals"])
        no += len(local["offdiagonals"])
        assert touched[0] <= own[0] and touched[1] >= own[1]
    assert nd == len(sp["diagonals"]) and no == len(sp["offdiagonals"])
    assert D.balanced_cuts([1, 1, 1, 1], 2) == [0, 2, 4]
    bp = bsm.synthetic.config1(n=2000, nblocks=90, bs=16)
    nb, prev_hi = 0, 0
    for r in range(4):
        local, own, touched = D.split_blocksparse(bp, r, 4)
        nb += len(local["blocks"])
        assert own[0] == prev_hi + 1 and touched[0] <= own[0] and touched[1] >= own[1]
        prev_hi = own[1]
        for rows in local["rowindices"]:
            assert own[0] <= int(np.min(rows)) <= own[1]
    assert nb == len(bp["blocks"]) and prev_hi == 2000
    cp = bsm.synthetic.config2(n=8000, nblocks=500)
    for r in range(3):
        local, own = D.split_vbcrs(cp, r, 3, axis=1)
        for cs, b in zip(local["colstart"], local["blocks"]):
            assert own[0] <= cs and cs + b.shape[1] - 1 <= own[1]


def test_one_rank_loopback_rehearsal_logic():
    """`RowPartitioned(loopback=...)`: every collective / point-to-point branch against the rank itself (tests/_loopback.py).
    Here on the CPU over gloo (self send / recv replaced by an in-process copy: gloo has no pair to the own rank) with the
    image interpreter as local product -- the logic of what `-m gpu` runs over RCCL on the one GPU of the test box."""
    import _loopback
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_loopback.run, args=("gloo", _free_port(), q))
    p.start()
    status, res, extra = q.get(timeout=400)
    p.join(timeout=120)
    assert status == "ok", res
    assert len(res) >= 20 and all(e < 1e-12 for _, e in res), res
    assert p.exitcode == 0
