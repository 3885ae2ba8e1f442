"""Ragged haplotypes + realigned tracks through the native ring, against fixed-length rows (one JSON line per leg, then a summary).

cfg4-shaped legs: 16 regions x 64 samples of 131 072 bp, ploidy 2, SNPs + indels, one-hot + bytes, one BigWig-like track;
batches of 256 windows, 4 per epoch.  Per batch through the ring: fixed haplotypes, fixed haplotypes + track, ragged haplotypes,
ragged haplotypes + track.

Mixed-length leg: 64 regions of 200 - 20 000 bp x 32 samples x ploidy 2 = 4 096 rows in one batch, the track call
(gvl_tracks_batch, HIP events) and the ring's batch on the rows x chunks grid whose chunk-waves past their row's end exit (the
default) and through the chunk list (DBG_CHUNK_LIST), with the waves each schedule launches and the waves that have work.

    python tools/ragged_tracks_bench.py [--epochs 11] [--out FILE]      (one JSON line; profiles/r07_ragged_tracks.jsonl holds three runs)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHUNK_LIST = -(1 << 31)     # DBG_CHUNK_LIST
LIST_WGS = 2048          # CHUNK_LIST_WGS, gvl_tracks_kernels.inc


def make_data(rng, R, S, P, lens, contig=256 << 20):
    from genvarloader_amd import HapsDevice, synth

    st = synth.make_static(rng, (contig,), indel_frac=0.15)
    full_regions, go, gv = synth.make_grid(rng, st, R, S, P, int(max(lens)))
    full_regions = full_regions.copy()
    full_regions[:, 2] = full_regions[:, 1] + np.asarray(lens, np.int32)
    starts, ends, vals, offs = [], [], [], [0]
    for r in range(R):
        q0, q1 = int(full_regions[r, 1]), int(full_regions[r, 2])
        n = (q1 - q0 + 200) // 33 + 8
        w = rng.geometric(1 / 25, size=(S, n))
        g = rng.geometric(1 / 8, size=(S, n))
        for s_ in range(S):
            s0 = np.cumsum(w[s_] + g[s_]) - w[s_] + q0 - 100
            m = s0 < q1 + 50
            starts.append(s0[m]); ends.append((s0 + w[s_])[m]); vals.append((rng.random(int(m.sum())) * 8).astype(np.float32))
            offs.append(offs[-1] + int(m.sum()))
    tracks = {"cov": (np.concatenate(starts).astype(np.int32), np.concatenate(ends).astype(np.int32), np.concatenate(vals),
                      np.asarray(offs, np.int64))}
    dev = HapsDevice(ref=st.ref, ref_offsets=st.ref_offsets, v_starts=st.v_starts, ilens=st.ilens, alt_alleles=st.alt_alleles,
                     alt_offsets=st.alt_offsets, geno_offsets=go, geno_v_idxs=gv, pad_char=st.pad_char, device="cuda:0")
    return dev, full_regions, tracks


def ring_ms(torch, ds, batch_size, epochs):
    """ms per batch through the native ring (the consumer takes every batch and does nothing else); the first epoch is warm-up."""
    dl = ds.to_dataloader(batch_size=batch_size, shuffle=True, generator=torch.Generator().manual_seed(0))
    n_b, t0 = 0, None
    for e in range(epochs):
        dl.set_epoch(e)
        for _ in dl:
            n_b += 1 if e > 0 else 0
        torch.cuda.synchronize()
        if e == 0:
            t0 = time.perf_counter()
    return 1e3 * (time.perf_counter() - t0) / max(n_b, 1)


def cfg4_legs(torch, epochs):
    from genvarloader_amd.loader import DeviceHapsDataset, DeviceHapsTracksDataset

    R, S, P, L = 16, 64, 2, 131072
    dev, full_regions, tracks = make_data(np.random.default_rng(20261015), R, S, P, [L] * R)
    out = {}
    for name, ol, tr in [("fixed_haps", L, False), ("fixed_haps_track", L, True), ("ragged_haps", -1, False), ("ragged_haps_track", -1, True)]:
        if tr:
            ds = DeviceHapsTracksDataset(dev, full_regions, S, P, tracks=tracks, output_length=ol, onehot=True, haps=True)
        else:
            ds = DeviceHapsDataset(dev, full_regions, S, P, output_length=ol, onehot=True, haps=True)
        out[name] = ring_ms(torch, ds, 256, epochs)
        print(json.dumps({"leg": "cfg4." + name, "ms_per_batch": round(out[name], 4)}), flush=True)
        del ds
        torch.cuda.empty_cache()
    inc_f = out["fixed_haps_track"] - out["fixed_haps"]
    inc_r = out["ragged_haps_track"] - out["ragged_haps"]
    return {"track_increment_fixed_ms": round(inc_f, 4), "track_increment_ragged_ms": round(inc_r, 4),
            "ragged_over_fixed": round(inc_r / inc_f, 3) if inc_f > 0 else None}


def mixed_leg(torch, epochs, reps=30):
    from genvarloader_amd import _lib, device
    from genvarloader_amd.loader import DeviceHapsDataset, DeviceHapsTracksDataset

    R, S, P = 64, 32, 2
    rng = np.random.default_rng(7)
    lens = rng.integers(200, 20001, R)
    dev, full_regions, tracks = make_data(rng, R, S, P, lens)
    lib = _lib.load()
    ds = DeviceHapsTracksDataset(dev, full_regions, S, P, tracks=tracks, output_length=-1, onehot=False, haps=True)
    ds_h = DeviceHapsDataset(dev, full_regions, S, P, output_length=-1, onehot=False, haps=True)
    # one batch of every (region, sample): 4 096 rows; the track call timed alone
    idx = np.arange(R * S)
    r_idx, s_idx = np.unravel_index(idx, (R, S))
    regions = np.ascontiguousarray(full_regions[r_idx])
    goi = np.ravel_multi_index((r_idx[:, None], s_idx[:, None], np.arange(P)), (R, S, P))
    shifts = np.zeros_like(goi, dtype=np.int32)
    to_rc = np.repeat(regions[:, 3] == -1, P).astype(np.uint8)
    bt = dev.prepare_batch(regions, shifts, goi, -1, to_rc=to_rc)
    oo, _, _ = dev.hap_offsets(bt)
    lens_k = np.diff(oo.cpu().numpy())
    K, mrl = int(lens_k.size), ds.max_row_len()
    chunk_len = 2048 if mrl > 2048 else mrl
    chunks = -(-mrl // chunk_len)
    work = int((-(-lens_k // chunk_len)).sum())
    waves = {"rows": K, "max_row_len": mrl, "chunks_per_row_bound": chunks, "waves_with_work": work,
             "grid_waves_launched": -(-K // 4) * 4 * chunks, "list_waves_launched": min(-(-K * chunks // 4), LIST_WGS) * 4}
    res = {"waves": waves}
    for name, flags in [("bound_grid", 0), ("chunk_list", CHUNK_LIST)]:
        lib.gvl_set_debug_flags(flags)
        call = lambda: device.tracks_batch(dev, regions, shifts, goi, idx, ds._track_sets, [0.0], 0, 0, to_rc, output_length=-1,
                                           out_offsets=oo, max_row_len=mrl, scratch_stride=ds._stride)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(reps):
            call()
        ev1.record()
        torch.cuda.synchronize()
        res[name + "_call_ms"] = round(ev0.elapsed_time(ev1) / reps, 4)
        res[name + "_ring_ms_per_batch"] = round(ring_ms(torch, ds, R * S, epochs), 4)
        print(json.dumps({"leg": "mixed." + name, "call_ms": res[name + "_call_ms"],
                          "ring_ms_per_batch": res[name + "_ring_ms_per_batch"]}), flush=True)
    lib.gvl_set_debug_flags(-1)
    res["ragged_haps_ring_ms_per_batch"] = round(ring_ms(torch, ds_h, R * S, epochs), 4)
    res["list_speedup_call"] = round(res["bound_grid_call_ms"] / res["chunk_list_call_ms"], 3)
    res["list_speedup_ring"] = round(res["bound_grid_ring_ms_per_batch"] / res["chunk_list_ring_ms_per_batch"], 3)
    res["default"] = "chunk_list" if min(res["list_speedup_call"], res["list_speedup_ring"]) >= 1.1 else "bound_grid"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    summary = {"cfg4": cfg4_legs(torch, a.epochs), "mixed": mixed_leg(torch, a.epochs), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(summary)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
