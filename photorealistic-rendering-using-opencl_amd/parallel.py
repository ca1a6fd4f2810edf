"""Multi-GPU plumbing: how the frame is partitioned over ranks and how the pieces are merged.

The path shards with no data-path exchange: every pixel is independent (its state, RNG keying and
output depend only on its own global coordinates and the frame number), so each rank renders its
own rows and ONE collective at the end puts the framebuffer together on rank 0: a gather of
the ranks' row tiles to rank 0 (RCCL over xGMI when the backend is nccl), scattered into place by row index.
Moving the rows themselves is lossless for every bit pattern (a sum of zero-padded frames would turn
-0.0 into +0.0) and moves each pixel once instead of N times.
Rows are dealt in interleaved blocks of 16 (prt_set_row_blocks) so the ranks get equal shares of
the expensive middle of the picture.
"""
import numpy as np

from ._capi import DENOISE_RECORD_FLOATS as RECORD_FLOATS, MOTION_FLOATS

BLOCK_ROWS = 16


def rows_of_rank(height, world, rank, block=BLOCK_ROWS):
    """global row indices owned by `rank`, in local order (matches prt_set_row_blocks)"""
    rows = np.arange(height)
    return rows[(rows // block) % world == rank]


def max_rows_per_rank(height, world, block=BLOCK_ROWS):
    return max(len(rows_of_rank(height, world, r, block)) for r in range(world))


def gather_rows_on_rank0(tile, height, width, world, dist, block=BLOCK_ROWS):
    """tile: (max_rows_per_rank, width, ...) torch tensor of any trailing shape and dtype, this rank's rows first (padding rows are ignored).
    ONE collective: a gather to rank 0 (every pixel crosses a link once; the rows themselves travel: every bit pattern survives).  Returns
    the full (height, width, ...) tensor on rank 0, None on the other ranks; with one rank the tile's rows."""
    import torch
    if world == 1 or dist is None or not dist.is_initialized():
        return tile[:height]
    rank = dist.get_rank()
    pieces = [torch.empty_like(tile) for _ in range(world)] if rank == 0 else None
    dist.gather(tile.contiguous(), gather_list=pieces, dst=0)
    if rank != 0:
        return None
    full = torch.empty((height, width) + tuple(tile.shape[2:]), dtype=tile.dtype, device=tile.device)
    for r in range(world):
        rows = rows_of_rank(height, world, r, block)
        idx = torch.as_tensor(np.asarray(rows), dtype=torch.long, device=tile.device)
        full.index_copy_(0, idx, pieces[r][:len(rows)])
    return full


def merge_on_rank0(tile, height, width, world, dist):
    """tile: (max_rows_per_rank, width, 4) float32 torch tensor, this rank's rows first (padding rows are ignored).
    ONE collective: a gather to rank 0 (every pixel crosses a link once).  Returns the full (height, width, 4) tensor on rank 0,
    None on the other ranks."""
    return gather_rows_on_rank0(tile, height, width, world, dist)


def pack_motion_tile(records, motion):
    """(rows, width, 16) records and (rows, width, 4) motion -> ONE (rows, width, 20) tile: what a rank sends when the motion plane travels
    with the records, so that there is still exactly one collective"""
    import torch
    return torch.cat([records, motion], dim=-1).contiguous()


def split_motion_tile(full):
    """the gathered (height, width, 20) tile -> the two contiguous buffers the filter reads: (height, width, 16) records, (height, width, 4) motion"""
    return full[..., :RECORD_FLOATS].contiguous(), full[..., RECORD_FLOATS:RECORD_FLOATS + MOTION_FLOATS].contiguous()


def denoise_on_rank0(renderer, height, width, world, dist, cam=None, temporal=False, motion=False, **params):
    """The denoised frame of a render dealt over `world` ranks in row blocks (prt_set_row_blocks(width, height, BLOCK_ROWS, world, rank) on
    every rank, rendered, guides rendered): every rank exports its records (Renderer.export_denoise_inputs) into a
    (max_rows_per_rank, width, 16) tensor, ONE collective gathers them to rank 0 -- instead of the framebuffer's gather, not on top of it -- and
    rank 0's context filters the whole frame (Renderer.denoise_records, or with temporal=True denoise_records_temporal with `cam`, the frame's
    camera).  motion=True (needs temporal=True and Renderer.set_motion on every rank): every rank also exports its motion plane
    (Renderer.export_motion) and sends both as one (rows, width, 20) tile -- still one collective --, which rank 0 splits into the two
    contiguous buffers of prt_denoise_records_temporal_motion.  params: the keywords of Renderer.denoise / denoise_temporal.  Returns the (height, width, 4) float32 tensor on rank 0's device,
    None on the other ranks.  The bits are those of prt_denoise on one whole-frame context.  A temporal response
    (Renderer.set_temporal_response) needs no argument here: the setting is rank 0's context's, whose record history the call uses."""
    import torch
    if temporal and cam is None:
        raise ValueError("denoise_on_rank0: temporal=True needs the frame's camera")
    if motion and not temporal:
        raise ValueError("denoise_on_rank0: motion=True needs temporal=True (the motion plane feeds the reprojection)")
    rank = dist.get_rank() if (world > 1 and dist is not None and dist.is_initialized()) else 0
    device = torch.device("cuda", torch.cuda.current_device())
    tile = torch.zeros((max_rows_per_rank(height, world), width, 16), dtype=torch.float32, device=device)
    assert renderer.rows == len(rows_of_rank(height, world, rank)) and renderer.width == width, "the renderer's frame part is not this rank's"
    # torch's work runs on torch's current stream, the library's on the context's (its own unless Renderer.set_stream made them one): each
    # side starts behind the other's finished work
    torch.cuda.current_stream().synchronize()
    renderer.export_denoise_inputs(tile)
    if motion:
        mtile = torch.zeros((tile.shape[0], width, MOTION_FLOATS), dtype=torch.float32, device=device)
        renderer.export_motion(mtile)
    renderer.synchronize()
    if motion:
        tile = pack_motion_tile(tile, mtile)
        torch.cuda.current_stream().synchronize()
    records = gather_rows_on_rank0(tile, height, width, world, dist)
    if rank != 0:
        return None
    plane = None
    if motion:
        records, plane = split_motion_tile(records)
    records = records.contiguous()
    torch.cuda.current_stream().synchronize()
    out = torch.empty((height, width, 4), dtype=torch.float32, device=device)
    if temporal:
        return renderer.denoise_records_temporal(records, width, height, cam, out=out, motion=plane, **params)
    return renderer.denoise_records(records, width, height, out=out, **params)
