"""Ragged haplotypes + realigned tracks (the reference's default ``output_length="ragged"``, ``_reconstruct.py:183-203``): every
track row as long as its haplotype, track t's block laid out at the haplotypes' row offsets.  Each block is checked bit for bit
against the oracle's ``intervals_and_realign_track_fused`` over the same offsets."""

import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_loader import _grid_dataset

R, S = 6, 4
# the five fill strategies with their parameters; FlankSample (3) pinned to a seed
FILLS = [(0, 0.0), (1, 0.0), (2, 3.0), (3, 6.0), (4, 0.0)]
CHUNK_LIST = -(1 << 31)             # DBG_CHUNK_LIST: ragged rows through their chunk list (1-D launches), not the rows x chunks grid
TRACK_DBG = [0, 1024, 8, 8192, 2097152, 4194304, 1073741824, CHUNK_LIST, CHUNK_LIST | 8, CHUNK_LIST | 4194304, CHUNK_LIST | 1073741824]
TRACK_DBG_IDS = ["default", "painter-without-bucket-index", "scalar-walk", "painter-image-path", "intervals-without-window",
                 "painter-first", "general-track-kernel", "chunk-list", "chunk-list-scalar-walk", "chunk-list-painter-first",
                 "chunk-list-general-track-kernel"]


def _lengths(shape, rng):
    if shape == "one-chunk":
        return rng.integers(150, 1500, R)
    if shape == "several-chunks":
        return rng.integers(4500, 5200, R)
    return np.array([200, 6500, 900, 3100, 4800, 350])[:R]            # mixed


def _dataset(seed, P, shape):
    from genvarloader_amd import HapsDevice

    rng = np.random.default_rng(seed)
    lens = _lengths(shape, rng)
    st, full_regions, go, gv = _grid_dataset(seed, R, S, P, int(lens.max()), indel_frac=0.5, slack=30)
    full_regions = full_regions.copy()
    full_regions[:, 2] = full_regions[:, 1] + lens.astype(np.int32)
    full_regions[:, 3] = np.where(np.arange(R) % 2 == 0, 1, -1)            # negative-strand rows are reversed
    dev = HapsDevice(ref=st.ref, ref_offsets=st.ref_offsets, v_starts=st.v_starts, ilens=st.ilens,
                     alt_alleles=st.alt_alleles, alt_offsets=st.alt_offsets, geno_offsets=go, geno_v_idxs=gv,
                     pad_char=st.pad_char)
    return st, full_regions, go, gv, dev


def _intervals(rng, full_regions, n_lists, per_region, overlap):
    starts, ends, vals, offs = [], [], [], [0]
    for li in range(n_lists):
        r = li // per_region
        pos = int(full_regions[r, 1]) - int(rng.integers(0, 60))
        while pos < int(full_regions[r, 2]) + 40:
            w, gap = int(rng.geometric(1 / 25)), int(rng.integers(0, 6))
            s0 = pos + gap
            starts.append(s0); ends.append(s0 + w + (int(rng.integers(0, 30)) if overlap else 0)); vals.append(float(rng.random() * 5))
            pos = s0 + w
        offs.append(len(starts))
    return np.array(starts, np.int32), np.array(ends, np.int32), np.array(vals, np.float32), np.array(offs, np.int64)


def _tracks(seed, full_regions):
    """A BigWig-like track (tile_complete), one with overlapping intervals (not), a region-level one and one with its own fill."""
    rng = np.random.default_rng(seed + 100)
    t = {"cov": _intervals(rng, full_regions, R * S, S, False), "ovl": _intervals(rng, full_regions, R * S, S, True)}
    a, e, v, o = _intervals(rng, full_regions, R, 1, False)
    t["reg"] = dict(starts=a, ends=e, values=v, offsets=o, region_level=True)
    a, e, v, o = _intervals(rng, full_regions, R * S, S, False)
    t["own"] = dict(starts=a, ends=e, values=v, offsets=o, fill=(2, 7.5))
    return t


def _spec(tr):
    if isinstance(tr, dict):
        return tr["starts"], tr["ends"], tr["values"], tr["offsets"], tr.get("fill"), bool(tr.get("region_level", False))
    return (*tr, None, False)


def _expected(oracle, st, go, gv, P, idx, regions, out_offsets, to_rc, tr, strategy, param, seed):
    """One track's block: the oracle's paint + realign over the haplotype offsets."""
    r_idx, s_idx = np.unravel_index(idx, (R, S))
    goi = np.ravel_multi_index((r_idx[:, None], s_idx[:, None], np.arange(P)), (R, S, P))
    shifts = np.zeros_like(goi, dtype=np.int32)
    diffs = oracle.get_diffs_sparse(goi, gv, go, st.ilens, None, None, regions[:, 1], regions[:, 2], st.v_starts)
    tlen = (regions[:, 2] - regions[:, 1]).astype(np.int64) - np.minimum(diffs.min(axis=1), 0)
    track_offsets = np.concatenate([[0], np.cumsum(tlen)]).astype(np.int64)
    a, e, v, io, fill, region_level = _spec(tr)
    if fill is not None:
        strategy, param = fill
    oi = (r_idx if region_level else idx).astype(np.int64)
    exp = np.zeros(int(out_offsets[-1]), np.float32)
    oracle.intervals_and_realign_track_fused(exp, out_offsets, regions, shifts, goi, gv, go, st.v_starts, st.ilens, oi, a, e, v, io,
                                             track_offsets, np.array([param]), strategy, seed, None, None, to_rc)
    return exp


@pytest.fixture
def dbg_flags(request):
    from genvarloader_amd import _lib

    _lib.load().gvl_set_debug_flags(int(request.param))
    yield int(request.param)
    _lib.load().gvl_set_debug_flags(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("dbg_flags", TRACK_DBG, ids=TRACK_DBG_IDS, indirect=True)
@pytest.mark.parametrize("shape", ["one-chunk", "several-chunks", "mixed"])
@pytest.mark.parametrize("P", [1, 2])
def test_tracks_batch_ragged_rows_match_oracle(oracle, dbg_flags, shape, P):
    """gvl_tracks_batch with output_length -1: track t's row k at out[t * stride + out_offsets[k] ..] for the haplotypes' offsets."""
    from genvarloader_amd import device
    from genvarloader_amd.loader import DeviceHapsTracksDataset

    st, full_regions, go, gv, dev = _dataset(61 + P, P, shape)
    tracks = _tracks(7, full_regions)
    ds = DeviceHapsTracksDataset(dev, full_regions, S, P, tracks=tracks, output_length=-1, onehot=False, haps=True)
    assert ds._tile_complete == [True, False, True, True]
    rng = np.random.default_rng(3)
    idx = rng.permutation(R * S)[:13]
    r_idx, s_idx = np.unravel_index(idx, (R, S))
    regions = np.ascontiguousarray(full_regions[r_idx])
    goi = np.ravel_multi_index((r_idx[:, None], s_idx[:, None], np.arange(P)), (R, S, P))
    shifts = np.zeros_like(goi, dtype=np.int32)
    to_rc = np.repeat(regions[:, 3] == -1, P).astype(np.uint8)
    bt = dev.prepare_batch(regions, shifts, goi, -1, to_rc=to_rc)
    oo, tm, _ = dev.hap_offsets(bt)
    out_offsets = oo.cpu().numpy()
    lens = np.diff(out_offsets)
    if shape == "mixed":
        assert lens.min() <= 2048 < lens.max()
    T = len(tracks)
    for strategy, param in FILLS:
        got = device.tracks_batch(dev, regions, shifts, goi, idx, ds._track_sets, [param], strategy, 11, to_rc, output_length=-1,
                                  out_offsets=oo, scratch_stride=ds._stride)
        assert got.shape == (T, len(idx) * P * int(lens.max()))
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for t, name in enumerate(tracks):
            exp = _expected(oracle, st, go, gv, P, idx, regions, out_offsets, to_rc, tracks[name], strategy, param, 11)
            np.testing.assert_array_equal(got[t, :out_offsets[-1]].view(np.uint32), exp.view(np.uint32),
                                          err_msg=f"{name} strategy {strategy}")


def _check_batch(oracle, st, go, gv, P, ds_h, tracks, batch, strategy, param, pinned, ring):
    idx = batch.idx.cpu().numpy()
    oo = batch.out_offsets.cpu().numpy()
    total = int(oo[-1])
    if ds_h is not None:
        ref = ds_h[torch.as_tensor(idx)]                   # the ragged haplotype dataset's batch
        np.testing.assert_array_equal(oo, ref.out_offsets.cpu().numpy())
        np.testing.assert_array_equal(batch.haps[:total].cpu().numpy(), ref.haps.cpu().numpy())
    if ring:
        assert batch.tracks.shape[1] >= total and int(batch.sizes[0]) == total
    else:
        assert batch.tracks.shape[1] == total
    regions = batch.regions.cpu().numpy()
    to_rc = np.repeat(regions[:, 3] == -1, P).astype(np.uint8)
    seed = pinned if pinned is not None else int(np.bitwise_xor.reduce(idx.astype(np.uint64)))
    got = batch.tracks[:, :total].contiguous().cpu().numpy()
    for t, name in enumerate(tracks):
        exp = _expected(oracle, st, go, gv, P, idx, regions, oo, to_rc, tracks[name], strategy, param, seed)
        np.testing.assert_array_equal(got[t].view(np.uint32), exp.view(np.uint32), err_msg=f"{name} strategy {strategy}")
    return len(idx)


@pytest.mark.gpu
@pytest.mark.parametrize("sizing", [0, 1], ids=["epoch-sizing", "group-sizing"])
def test_ragged_haps_tracks_dataset_matches_oracle(oracle, sizing):
    """DeviceHapsTracksDataset(output_length=-1): the native ring (group 1 and 4, threaded), the Python submit loop, a short last
    batch, two epochs (the second from the prefetched table); GVL_TUNE_RAGGED_SIZING off and on."""
    from genvarloader_amd import _lib
    from genvarloader_amd.loader import DeviceHapsDataset, DeviceHapsTracksDataset

    P = 2
    st, full_regions, go, gv, dev = _dataset(71, P, "mixed")
    tracks = _tracks(9, full_regions)
    ds_h = DeviceHapsDataset(dev, full_regions, S, P, output_length=-1, onehot=False, haps=True)
    lib = _lib.load()
    lib.gvl_set_tuning(_lib.TUNE_RAGGED_SIZING, sizing)
    try:
        lib.gvl_async_error(1)
        for strategy, param, pinned, python_loop, group, threaded in [(0, 0.0, None, False, 1, False), (3, 6.0, 5, False, 4, False),
                                                                      (4, 0.0, None, False, 1, True), (3, 6.0, None, True, 1, False)]:
            ds = DeviceHapsTracksDataset(dev, full_regions, S, P, tracks=tracks, strategy_id=strategy, param=param, base_seed=pinned,
                                         output_length=-1, onehot=False, haps=True)
            dl = ds.to_dataloader(batch_size=5, shuffle=True, generator=torch.Generator().manual_seed(2), python_loop=python_loop,
                                  group=group, threaded=threaded)
            for epoch in range(2):
                dl.set_epoch(epoch)
                seen = 0
                for batch in dl:
                    seen += _check_batch(oracle, st, go, gv, P, ds_h, tracks, batch, strategy, param, pinned, not python_loop)
                assert seen == R * S                                   # 24 = 4 batches of 5 + a short last one of 4
            del dl
        torch.cuda.synchronize()
        assert lib.gvl_async_error(1) == 0
    finally:
        lib.gvl_set_tuning(_lib.TUNE_RAGGED_SIZING, 0)


@pytest.mark.gpu
def test_ragged_track_rows_longer_than_the_slot_bound_are_reported(oracle):
    """A max_row_len below the longest row: the ring cuts haplotype and track rows alike (one set of offsets), reports the cut
    through gvl_async_error; gvl_tracks_batch given rows past its bound writes nothing past any track's capacity."""
    from genvarloader_amd import _lib, device
    from genvarloader_amd.loader import DeviceHapsTracksDataset

    P = 2
    st, full_regions, go, gv, dev = _dataset(81, P, "mixed")
    tracks = _tracks(13, full_regions)
    ds = DeviceHapsTracksDataset(dev, full_regions, S, P, tracks=tracks, output_length=-1, onehot=False, haps=True)
    true_bound = ds.max_row_len()
    cut = 3000
    assert true_bound > cut
    ds._max_row_len = cut
    lib = _lib.load()
    lib.gvl_async_error(1)
    n_seen = 0
    with pytest.raises(ValueError, match="max_row_len"):
        for batch in ds.to_dataloader(batch_size=5, shuffle=False):
            assert int(batch.sizes[1]) <= cut
            _check_batch(oracle, st, go, gv, P, None, tracks, batch, 0, 0.0, None, True)     # (track rows over the cut offsets)
            n_seen += 1
    assert n_seen == -(-R * S // 5)
    torch.cuda.synchronize()
    assert lib.gvl_async_error(1) == 0



@pytest.mark.gpu
@pytest.mark.parametrize("dbg_flags", [0, CHUNK_LIST], ids=["grid", "chunk-list"], indirect=True)
@pytest.mark.parametrize("case", ["total-fits", "total-over-capacity"])
def test_tracks_batch_rows_past_the_bound_write_nothing_past_the_capacity(dbg_flags, case):
    """gvl_tracks_batch given the haplotypes' UNCUT offsets with a max_row_len below the longest row: the rows are reported through
    gvl_async_error, and nothing is written past any track's batch * ploidy * max_row_len values -- also when the offsets' total
    exceeds that capacity (rows past it are clamped away), on either schedule."""
    from genvarloader_amd import _lib, device
    from genvarloader_amd.loader import DeviceHapsTracksDataset

    P, cut = 2, 3000
    st, full_regions, go, gv, dev = _dataset(81, P, "mixed")
    tracks = _tracks(13, full_regions)
    ds = DeviceHapsTracksDataset(dev, full_regions, S, P, tracks=tracks, output_length=-1, onehot=False, haps=True)
    lib = _lib.load()
    # regions 0, 1, 2, 5: one row of 6500 among short ones; regions 1, 1, 1, 4: rows of 6500 and 4800 only
    idx = np.array([0, 4, 8, 20] if case == "total-fits" else [4, 5, 6, 16], np.int64)
    r_idx, s_idx = np.unravel_index(idx, (R, S))
    regions = np.ascontiguousarray(full_regions[r_idx])
    goi = np.ravel_multi_index((r_idx[:, None], s_idx[:, None], np.arange(P)), (R, S, P))
    shifts = np.zeros_like(goi, dtype=np.int32)
    bt = dev.prepare_batch(regions, shifts, goi, -1)
    oo, _, _ = dev.hap_offsets(bt)
    o = oo.cpu().numpy()
    K = len(idx) * P
    assert np.diff(o).max() > cut
    assert (o[-1] <= K * cut) == (case == "total-fits")
    # (a guard as long as the whole uncut batch: even a write at every uncut offset would stay inside the buffer)
    T, G = len(tracks), max(4096, int(o[-1]))
    stride = K * cut + G
    out = torch.full((T, stride), float("nan"), dtype=torch.float32, device=dev.device)
    btc = dev.prepare_batch(regions, shifts, goi, -1, out_offsets=oo, max_row_len=cut)
    scr = torch.empty(int(lib.gvl_tracks_scratch_bytes(C.c_int64(len(idx)), C.c_int64(P), C.c_int64(ds._stride))), dtype=torch.uint8,
                      device=dev.device)
    oi = torch.as_tensor(idx, device=dev.device)
    torch.cuda.synchronize()
    lib.gvl_async_error(1)
    par = (C.c_double * 1)(0.0)
    _lib.check(lib.gvl_tracks_batch(C.byref(dev.c), C.byref(btc.c), C.c_void_p(oi.data_ptr()), ds._track_sets, C.c_int32(T), par,
                                    C.c_int64(0), C.c_uint64(0), C.c_void_p(out.data_ptr()), C.c_int64(stride), C.c_void_p(scr.data_ptr()),
                                    C.c_int64(ds._stride), device._stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gvl_async_error(1) != 0
    np.testing.assert_array_equal(oo.cpu().numpy(), o)           # (the caller's offsets are left alone)
    tail = out[:, K * cut:].cpu().numpy()
    assert np.isnan(tail).all()                                  # nothing past any track's max_row_len * rows capacity
    assert not np.isnan(out[:, :min(int(o[1]), cut)].cpu().numpy()).any()   # (the first row, inside the capacity, was written)
