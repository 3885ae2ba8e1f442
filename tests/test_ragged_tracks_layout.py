"""Host arithmetic of the ring's ragged haplotypes + tracks configuration (no GPU): the slot's tracks part holds
n_tracks x batch_size x ploidy x max_row_len f32, and the epoch table carries the scratch-track sizing next to the ragged offsets."""

import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from genvarloader_amd import _lib

    return _lib.load()


def test_ragged_tracks_slot_and_table_layout(lib):
    from genvarloader_amd import _lib

    up = lambda x: (x + 255) & ~255
    bs, P, T, M = 8, 2, 3, 500
    K = bs * P
    cfg = _lib.GvlLoaderConfig(n_regions=10, n_samples=4, ploidy=P, batch_size=bs, output_length=-1, max_row_len=M, want_haps=1,
                               deterministic=1, n_tracks=T, scratch_stride=700)
    parts = (C.c_int64 * _lib.LOADER_SLOT_PARTS)()
    lib.gvl_loader_slot_bytes.restype = C.c_int64
    assert int(lib.gvl_loader_slot_bytes(C.byref(cfg), parts)) > 0
    p = [int(x) for x in parts]
    assert p[1] - p[0] == 0 and p[2] - p[1] == up(K * M)              # the haplotype bytes: K * max_row_len
    assert p[10] - p[9] == up(4 * T * K * M)                           # track t at t * K * max_row_len
    lib.gvl_tracks_scratch_bytes.restype = C.c_int64
    assert p[11] - p[10] == up(int(lib.gvl_tracks_scratch_bytes(C.c_int64(bs), C.c_int64(P), C.c_int64(700))))
    n, nb = 100, 13
    po = (C.c_int64 * _lib.LOADER_TABLE_PARTS)()
    lib.gvl_loader_table_bytes.restype = C.c_int64
    total = int(lib.gvl_loader_table_bytes(C.byref(cfg), C.c_int64(n), po))
    po = [int(x) for x in po]
    assert po[6] - po[5] == up(8 * (n + nb))                           # every batch's scratch-track offsets
    assert total - po[9] == up(8 * nb * (K + 1 + 2))                   # ... and its ragged row offsets + {total, longest}

