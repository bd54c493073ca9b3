"""CPU suite: the process-per-GPU layer (blocksparsematrices.jl_amd/distributed.py) on the layout-edge operators of
tests/_fuzz.py -- block rows that start anywhere and overlap the next part's rows, scattered and unsorted index lists,
parts without blocks, rectangular sizes.

1. the row partition and the splits as plain properties (no process group): three kinds x 12 operators x 2, 3, 5, 8 parts;
2. products over `gloo` with worlds 2, 3, 5, several operators inside one process group per spawn, the packed-image
   interpreter as local product (tests/_distworker.py, the rank process of tests/test_distributed_cpu.py), against the
   CPU oracle on the whole operator at that file's bound, 1e-12;
3. the operators of (2) reach every partition edge of _fuzz.partition_features that applies to their kind (asserted;
   one DISTSTAT line per kind: docs/experiments_r14.md quotes them)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from _common import BLOCK_KEYS, nblocks  # noqa: E402
from _distworker import fuzz_problems, spawn  # noqa: E402
from _fuzz import block_lists, partition_features, partition_rule, squared  # noqa: E402

KINDS = ["blocksparse", "vbcrs", "symmetric"]
WORLDS = (2, 3, 5)
COUNT = 8  # operators per spawn
# the edges a kind can reach: blocks go with the owner of their smallest row, so only the column lists of symmetric
# off-diagonal blocks reach rows BELOW a part; symmetric operators are square
APPLICABLE = {"vbcrs": {"empty_part", "halo_above", "crossing_block", "tall", "wide"},
              "blocksparse": {"empty_part", "halo_above", "tall", "wide"},
              "symmetric": {"empty_part", "halo_below", "halo_above"}}
def _rows_written(p):
    """the hulls (lo, hi) of the rows every block of p writes under op N (symmetric: of the column lists too)"""
    rh, ch, _, _ = block_lists(p)
    spans = [h for h in rh if h is not None] + ([h for h in ch if h is not None] if p["kind"] == "symmetric" else [])
    return spans


@pytest.mark.parametrize("kind", KINDS)
def test_partition_and_splits_on_layout_edge_operators(kind):
    from bsm_amd import distributed as D
    from bsm_amd import matrices as M
    checked = 0
    for prob in fuzz_problems(kind, np.float64, 12):
        nr = prob["size"][0]
        rh, ch, keys, weights = block_lists(prob)
        for parts in (2, 3, 5, 8):
            part, own = M.partition_rows(nr, keys, weights, parts)
            rpart, rown = partition_rule(nr, keys, weights, parts)
            assert np.array_equal(part, rpart) and own == rown, (kind, parts, own, rown)
            # the own ranges tile 1 .. nrows, in order
            nxt = 1
            for lo, hi in own:
                assert lo == nxt or hi == lo - 1, own
                assert hi >= lo - 1
                nxt = hi + 1 if hi >= lo else nxt
            assert nxt == nr + 1, own
            seen = 0
            for r in range(parts):
                if kind == "vbcrs":
                    local, o = D.split_vbcrs(prob, r, parts)
                    touched = D.touched_range(local, o)
                else:
                    local, o, touched = (D.split_blocksparse if kind == "blocksparse" else D.split_symmetric)(prob, r, parts)
                    assert touched == D.touched_range(local, o)
                assert o == own[r]
                seen += nblocks(local)  # (every block in exactly one part: the parts' counts are those of `part`)
                assert nblocks(local) == int(np.sum(part == r))
                lrh, lch, lkeys, _ = block_lists(local)
                assert all(o[0] <= k <= o[1] for k, h in zip(lkeys, lrh) if h is not None), (kind, parts, r)
                assert touched[0] <= o[0] and touched[1] >= o[1] or o[1] < o[0]
                for lo, hi in _rows_written(local):
                    assert touched[0] <= lo and hi <= touched[1], (kind, parts, r, touched, (lo, hi))
                # ---- split_interior -----------------------------------------------------------------------------
                interior, boundary, bt, bx = D.split_interior(local, o)
                assert nblocks(interior) + nblocks(boundary) == nblocks(local)
                for k in BLOCK_KEYS:  # interior + boundary = local, block by block
                    ids = sorted(id(b) for b in local.get(k, ()))
                    assert sorted([id(b) for b in interior.get(k, ())] + [id(b) for b in boundary.get(k, ())]) == ids
                irh, ich, _, _ = block_lists(interior)
                for hr, hc in zip(irh, ich):
                    if hr is not None and hc is not None:  # (a block without rows or columns reads and writes nothing)
                        assert o[0] <= hr[0] and hr[1] <= o[1] and o[0] <= hc[0] and hc[1] <= o[1], (kind, parts, r)
                brh, bch, _, _ = block_lists(boundary)
                assert all(hr is not None and hc is not None for hr, hc in zip(brh, bch)), "an empty block became boundary"
                sym = kind == "symmetric"
                wr = brh + (bch if sym else [])
                rd = bch + (brh if sym else [])
                empty = (o[0], o[0] - 1)
                assert bt == ((min(h[0] for h in wr), max(h[1] for h in wr)) if wr else empty)
                assert bx == ((min(h[0] for h in rd), max(h[1] for h in rd)) if rd else empty)
                checked += 1
            assert seen == nblocks(prob)
    assert checked == 12 * (2 + 3 + 5 + 8)


def test_column_partition_hull_of_vbcrs():
    """split_vbcrs(axis=1): the blocks go by their first column, `touched_range(..., axis=1)` is the column hull"""
    from bsm_amd import distributed as D
    crossing = 0
    for prob in fuzz_problems("vbcrs", np.float64, 12):
        for parts in WORLDS:
            seen, nxt = 0, 1
            for r in range(parts):
                local, own = D.split_vbcrs(prob, r, parts, axis=1)
                t = D.touched_range(local, own, axis=1)
                seen += len(local["blocks"])
                if own[1] >= own[0]:
                    assert own[0] == nxt
                    nxt = own[1] + 1
                for c, b in zip(local["colstart"], local["blocks"]):
                    assert own[0] <= c <= own[1] and t[0] <= c and c + b.shape[1] - 1 <= t[1]
                    crossing += c + b.shape[1] - 1 > own[1]
            assert seen == len(prob["blocks"]) and nxt == prob["size"][1] + 1
    assert crossing > 0


CASES = [(k, "float64", "square") for k in KINDS] + [("symmetric", "complex128", "square"),
                                                     ("vbcrs", "float64", "rect"), ("blocksparse", "float64", "rect")]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("kind,dtype,mode", CASES)
def test_products_over_gloo_on_layout_edge_operators(kind, dtype, mode, world):
    """One spawn per case, COUNT operators inside the one process group.  "square": every leg of the rank process (both
    gather modes, partitioned x, the overlapped halo / all-gather exchange, mul_multi), complex symmetric operators under
    op T and C too; "rect": the operators as drawn -- op N with full x, op T across the row partition (reduce-scatter /
    all-reduce) and, VBCRS, op T on the column partition."""
    status, errs, own, touched, codes = spawn(("fuzz", kind, dtype, COUNT, mode), world)
    assert status == "ok", errs
    print("DISTPROD {} {} {} world {} products {} worst {:.3e}".format(kind, dtype, mode, world, len(errs), max(errs)))
    assert len(errs) >= COUNT * 8
    assert all(e < 1e-12 for e in errs), " ".join("%.2e" % e for e in errs)
    assert all(c == 0 for c in codes)


@pytest.mark.parametrize("kind", KINDS)
def test_the_operators_reach_every_partition_edge(kind):
    """the coverage condition of the product tests above, over the (operator, world) pairs they run: the rectangular
    edges on the operators as drawn, the others on either form (squaring changes no row partition)"""
    reached, pairs, ranks_empty, ranks_halo = set(), {}, 0, 0
    for prob in fuzz_problems(kind, np.float64, COUNT):
        rh, ch, keys, weights = block_lists(prob)
        for world in WORLDS:
            f = partition_features(prob, world)
            assert partition_features(squared(prob), world) == f - {"tall", "wide"}
            reached |= f
            for name in f:
                pairs[name] = pairs.get(name, 0) + 1
            part, own = partition_rule(prob["size"][0], keys, weights, world)
            for r in range(world):
                mine = [b for b in range(len(keys)) if part[b] == r]
                ranks_empty += not mine
                hulls = [h for b in mine for h in ([rh[b]] + ([ch[b]] if kind == "symmetric" else [])) if h is not None]
                ranks_halo += any(h[0] < own[r][0] or h[1] > own[r][1] for h in hulls)
    print("DISTSTAT {} operators {} worlds {} pairs {} ranks_with_halo {} ranks_without_blocks {}".format(
        kind, COUNT, list(WORLDS), " ".join("%s=%d" % kv for kv in sorted(pairs.items())), ranks_halo, ranks_empty))
    assert reached >= APPLICABLE[kind], (kind, APPLICABLE[kind] - reached)
    assert reached <= APPLICABLE[kind], (kind, reached - APPLICABLE[kind])
