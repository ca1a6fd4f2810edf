"""parallel.gather_rows_on_rank0: the one collective that carries a frame's rows to rank 0, for any trailing shape -- here the 16-float
denoiser records of prt_export_denoise_inputs -- with world_size 2 and 4 over gloo on the CPU.  The contract: the rows themselves travel, so
the gathered frame is the single-rank frame word for word (-0.0, NaNs with a payload, denormals), and the padding rows of the uneven shares
never reach it."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG_NAME

W, C = 7, 16
CASES = {2: 41, 4: 73}                  # test_multi_rank's heights: the last block is short, the shares are uneven
POISON = 0xDEADBEEF                     # what the padding rows hold
SPECIAL = (0x80000000, 0x7FC12345, 0xFFC00ABC, 0x00000001, 0x807FFFFF)       # -0.0, two NaNs with a payload, two denormals


def _frame(H):
    """the single-rank frame as uint32 words [H, W, C]: random words, the special ones in the first pixels of every row, no POISON"""
    words = np.random.default_rng(H).integers(0, 2 ** 32, (H, W, C), dtype=np.uint32)
    words[words == POISON] = 0
    for k, s in enumerate(SPECIAL):
        words[:, k % W, (3 * k) % C] = s
    return words


def _tile(par, H, world, rank):
    rows = par.rows_of_rank(H, world, rank)
    padded = np.full((par.max_rows_per_rank(H, world), W, C), POISON, dtype=np.uint32)
    padded[:len(rows)] = _frame(H)[rows]
    return torch.from_numpy(padded.view(np.float32))


def _worker(rank, world, port, out_path, H):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    par = importlib.import_module(PKG_NAME + ".parallel")
    full = par.gather_rows_on_rank0(_tile(par, H, world, rank), H, W, world, dist)
    dist.barrier()
    assert (full is None) == (rank != 0)
    if rank == 0:
        assert full.shape == (H, W, C) and full.dtype == torch.float32
        np.save(out_path, full.numpy().view(np.uint32))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_gathered_records_equal_the_single_rank_frame(tmp_path, world):
    par = importlib.import_module(PKG_NAME + ".parallel")
    assert hasattr(par, "gather_rows_on_rank0") and hasattr(par, "denoise_on_rank0")
    H = CASES[world]
    assert len({len(par.rows_of_rank(H, world, r)) for r in range(world)}) > 1        # uneven shares: some tiles carry padding rows
    out = str(tmp_path / "gathered.npy")
    port = 31500 + (os.getpid() % 2000) + world
    mp.spawn(_worker, args=(world, port, out, H), nprocs=world, join=True)
    got = np.load(out)
    assert not (got == POISON).any()
    assert np.array_equal(got, _frame(H))
    for s in SPECIAL:
        assert (got == s).sum() >= H


def test_one_rank_returns_the_tiles_rows():
    par = importlib.import_module(PKG_NAME + ".parallel")
    H = 41
    tile = _tile(par, H, 1, 0)
    full = par.gather_rows_on_rank0(tile, H, W, 1, None)
    assert np.array_equal(full.numpy().view(np.uint32), _frame(H))
    # merge_on_rank0 is the same call for rgba tiles
    rgba = tile[..., :4].contiguous()
    assert np.array_equal(par.merge_on_rank0(rgba, H, W, 1, None).numpy().view(np.uint32), _frame(H)[..., :4])
