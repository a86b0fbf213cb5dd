"""hipstore::k_parity_update on HBM bdevs against parity_model.py (exact:
whole bdevs, sentinel margins included) and against the generic host path."""

import itertools

import numpy as np
import pytest

from oim_amd import _hipstore as hs

from parity_model import BLOCK, EXP, gf_mul
from test_parity_update import (LENGTH, Tracked, cancelling_and_refresh,
                                changed, tracked_set)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hs.gpu_available(),
                                                  reason="no HIP device")]

MAX_WGS = 2048
# Unroll tail, longest chain, skipped leading doublings, gaps in between.
TRACKED = [(1, [0]), (5, [0]), (5, [4]), (5, [1, 3]), (5, [0, 1, 2, 3, 4]),
           (32, [31]), (32, [0, 31])]


def hbm(name, block, blocks):
    return hs.create_hbm_bdev(name, block, blocks, device=0)


@pytest.mark.parametrize("which", ["p", "q", "pq"])
@pytest.mark.parametrize("k,tracked", TRACKED, ids=str)
def test_tracked_sets(k, tracked, which):
    tracked_set(hbm, k, tracked, which, True)


@pytest.mark.parametrize("granule", [512, 1024, 1536, 4096])
def test_slabs_and_bitmap(granule):
    n = 130  # three bitmap words, ragged; 1/2, 1, 1 1/2 and 4 slabs a granule
    t = Tracked(hbm, 4, n * granule, [1, 2])
    rng = np.random.default_rng(granule)
    planted = sorted({0, 63, 64, 65, n - 1} |
                     set(rng.choice(n, 30, replace=False).tolist()))
    positions = itertools.cycle([0, 15, 16, granule - 1])
    for j, g in enumerate(planted):
        t.change(1 + j % 2, g * granule + next(positions))
    r = t.update(granule=granule, max_report=1024)
    assert r["on_gpu"] and r["changed"] == changed(n, planted, 1024)
    t.check()


def test_grid_stride_wrap():
    # Uniform members have uniform parity; the scrub reads all of P and Q.
    n = 2 * MAX_WGS * 64 + 65
    g_a5 = int(gf_mul(EXP[1], np.array([0xA5], np.uint8))[0])
    fills = [0x3C, 0xA5, 0x3C ^ 0xA5, 0x3C ^ g_a5, 0xA5]
    d0, d1, p, q, base = (hbm(f"pu-wrap-{i}", BLOCK, n) for i in range(5))
    for bdev, fill in zip((d0, d1, p, q, base), fills):
        bdev.fill(0, fill, bdev.size_bytes)
    planted = [0, MAX_WGS * 64 - 1, MAX_WGS * 64, n - 1]
    for g, pos in zip(planted, [0, 15, 16, BLOCK - 1]):
        block = bytearray(d1.read(g * BLOCK, BLOCK))
        block[pos] ^= 0xFF
        d1.write(g * BLOCK, bytes(block))
    for want in (planted, []):  # the second call finds the base refreshed
        r = hs.parity_update([d0, d1], p, q, [None, base], max_report=4,
                             refresh=True)
        assert r["on_gpu"] and r["changed"] == changed(n, want)
        scrub = hs.parity_check([d0, d1], p, q)
        assert scrub["p"]["mismatched"] == scrub["q"]["mismatched"] == 0
        assert hs.bdev_diff(d1, base)["mismatched"] == 0


@pytest.mark.parametrize("refresh", [False, True])
def test_cancelling_and_refresh(refresh):
    assert cancelling_and_refresh(hbm, refresh)


@pytest.mark.parametrize("mixed", [False, True])
def test_two_paths_agree(mixed):
    # Malloc twins, or one malloc base: the generic path gives the same.
    gpu = Tracked(hbm, 3, LENGTH, [0, 1])
    host = Tracked(hbm, 3, LENGTH, [0, 1], {1: hs.create_malloc_bdev}) \
        if mixed else Tracked(hs.create_malloc_bdev, 3, LENGTH, [0, 1])
    results = []
    for t in (gpu, host):
        t.change(0, 17)
        t.change(1, 2 * BLOCK)
        results.append(t.update(refresh=True, granule=BLOCK))
        t.check(refreshed=True)
    assert results[0].pop("on_gpu") and not results[1].pop("on_gpu")
    assert results[0] == results[1]
    assert gpu.contents() == host.contents()
