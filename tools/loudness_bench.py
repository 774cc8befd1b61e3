#!/usr/bin/env python3
"""Time the loudness sink against the packed 48 kHz stereo decode.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed           decode_packed, 44.1 -> 48 kHz stereo (the yardstick)
  packed_tap       decode_packed, then loudness on its out and counts
  decode_loudness  decode_loudness (the samples stay in the handle)
and the device time of the resample stage (resample_time_us) and of the
loudness stage (loudness_time_us) of those steps.  The variants alternate in
rounds inside one process; every step is timed by device events on the call's
stream.  Work of the stage per sample and channel, from its code: the cascade
is 8 FMA + 2 products in double and runs twice (zero-state pass, true pass),
plus one FMA for y^2: 38 FLOP; bytes: the samples read twice (k_ld_local skips
a stream's last tile), the blocks written once.

Then one long stream: the tap on the device output of decode_long_packed
(20 000 generated frames to 48 kHz stereo, as tools/long_packed_bench.py),
n = 1, by the host clock around the synchronous calls, against that call's own
time.  Prints one JSON line (and writes it to --out).

  python tools/loudness_bench.py --out profiles/loudness.json
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_MEASURED = 6.29e12  # float4 copy, bytes/s
FLOP_PER_SAMPLE_CHANNEL = 2 * 18 + 2
HZ, CH = 48000, 2


def med(v):
    return float(np.median(np.array(v)))


def batch_part(a, torch, _gen, mp3_amd):
    n, F = a.streams, a.frames
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_loudness(True)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty((n, mp3_amd.packed_max_samples(HZ, F, 44100), CH), dtype=torch.float32, device="cuda")
    blocks = torch.empty((n, mp3_amd.loud_max_blocks(HZ, F, 44100)), dtype=torch.float32, device="cuda")
    bc = torch.zeros(n, dtype=torch.int32, device="cuda")
    peak = torch.zeros(n, dtype=torch.float32, device="cuda")
    variants = ("packed", "packed_tap", "decode_loudness")
    times = {k: [] for k in variants}
    stage = {k: {"resample": [], "loudness": []} for k in variants}
    fed = {}
    per = max(1, a.steps // a.rounds)

    def step(k):
        if k == "decode_loudness":
            dec.decode_loudness(d_in, offs, sizes, F, blocks=blocks, counts=bc, peak=peak, infos=infos,
                                stream=strm.cuda_stream)
            return
        dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)
        if k == "packed_tap":
            dec.loudness(out, counts, blocks=blocks, block_counts=bc, peak=peak, stream=strm.cuda_stream)

    for _ in range(a.rounds):
        for k in variants:
            for i in range(a.warmup + per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(strm)
                step(k)
                e1.record(strm)
                e1.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
                    stage[k]["resample"].append(dec.resample_time_us())
                    if k != "packed":
                        stage[k]["loudness"].append(dec.loudness_time_us())
            if k == "packed_tap":
                fed[k] = int(counts.cpu().numpy().astype(np.int64).sum())
                fed["blocks"] = int(bc.cpu().numpy().astype(np.int64).sum())
    res = {"shape": [n, F], "format": [HZ, CH], "steps": len(times["packed"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us"}
    base = med(times["packed"])
    for k in variants:
        t = np.array(times[k])
        res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                  "step_over_packed": float(np.median(t) / base), "resample_stage_median": med(stage[k]["resample"])}
        if k == "packed":
            continue
        ld, rs = med(stage[k]["loudness"]), med(stage[k]["resample"])
        samples = fed["packed_tap"]  # steady state: both feed a call's inputs' worth of samples
        flop = samples * CH * FLOP_PER_SAMPLE_CHANNEL
        byts = 2 * samples * CH * 4 + fed["blocks"] * 4
        res[k].update({"stage_median": ld, "stage_min": float(np.min(stage[k]["loudness"])),
                       "stage_over_resample_stage": ld / rs, "stage_share_of_step": ld / float(np.median(t)),
                       "stage_ns_per_sample": ld * 1e3 / max(samples, 1), "samples_per_call": samples,
                       "stage_fp64_flop_per_s": flop / (ld * 1e-6), "stage_bytes_per_s": byts / (ld * 1e-6),
                       "stage_share_of_measured_hbm": byts / (ld * 1e-6) / HBM_MEASURED})
    return res


def long_part(a, torch, _gen, mp3_amd):
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_loudness(True)
    out = torch.empty((mp3_amd.long_packed_bound(data, HZ), CH), dtype=torch.float32, device="cuda")
    H = (HZ + 5) // 10
    blocks = torch.empty((1, out.shape[0] // H + 1), dtype=torch.float32, device="cuda")
    bc = torch.zeros(1, dtype=torch.int32, device="cuda")
    peak = torch.zeros(1, dtype=torch.float32, device="cuda")
    lufs = torch.zeros(1, dtype=torch.float32, device="cuda")
    t_long, t_tap, t_stage, t_gate = [], [], [], []
    n = 0
    for i in range(a.warmup + a.long_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = dec.decode_long_packed(d_in, HZ, CH, segment_frames=32, out=out, gapless=True)
        t1 = time.perf_counter()
        n = int(len(r[0]))
        cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dec.loudness(out[None], cnt, blocks=blocks, block_counts=bc, peak=peak, flush=True)
        dec.sync()
        t3 = time.perf_counter()
        dec.integrated_lufs(blocks, bc, lufs=lufs)
        dec.sync()
        t4 = time.perf_counter()
        if i >= a.warmup:
            t_long.append((t1 - t0) * 1e6)
            t_tap.append((t3 - t2) * 1e6)
            t_gate.append((t4 - t3) * 1e6)
            t_stage.append(dec.loudness_time_us())
    return {"frames": a.long_frames, "out_samples": n, "blocks": int(bc.cpu()[0]), "lufs": float(lufs.cpu()[0]),
            "peak": float(peak.cpu()[0]), "decode_long_packed_call_median": med(t_long), "tap_call_median": med(t_tap),
            "tap_stage_median": med(t_stage), "gate_call_median": med(t_gate),
            "tap_call_over_decode_long_packed": med(t_tap) / med(t_long),
            "tap_stage_ns_per_sample": med(t_stage) * 1e3 / max(n, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--long-frames", type=int, default=20000)
    ap.add_argument("--long-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    res = batch_part(a, torch, _gen, mp3_amd)
    res["long"] = long_part(a, torch, _gen, mp3_amd)
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
