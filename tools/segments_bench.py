#!/usr/bin/env python3
"""Time the segment sink against the packed 48 kHz stereo decode, the resample
stage, the true-peak tap and apply_gain.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed           decode_packed, 44.1 -> 48 kHz stereo (the yardstick)
  decode_segments  decode_segments: the same into handle-owned samples, then
                   the stage
  segments         the stage alone on the packed out, every slot at -40 dBFS
                   (the generator's streams are mostly active)
  segments_median  the stage alone, every slot at the corpus's median hop
                   energy: the masks flip often, the emit kernel's worst case
  segments_wide    the stage alone on the same samples at the stride
                   decode_segments gives its rows (the worst case over the
                   input rates, 2.76 x as far apart): twice the tiles per
                   stream, half of them empty
  true_peak        the true-peak tap alone: it reads the same bytes with more
                   arithmetic
  apply_f32        apply_gain alone, float32 to float32: it reads the bytes the
                   stage reads (and writes as many); the rate it reaches is the
                   yardstick of the stage's read
and the device time of the segment stage (segment_time_us) next to the
resample stage (resample_time_us).  The variants alternate in rounds inside
one process; every step is timed by device events on the call's stream.  No
call flushes.  The stage reads 4 bytes per sample and channel and writes a
few words per stream.

Then one long stream: the stage on the device output of decode_long_packed
(20 000 generated frames to 48 kHz stereo, as tools/limiter_bench.py), n = 1,
flushed, by the host clock around the synchronous calls, against that call's
own time.  Prints one JSON line (and writes it to --out).

  python tools/segments_bench.py --out profiles/segments.json
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
HZ, CH, H = 48000, 2, 480
VARIANTS = ("packed", "decode_segments", "segments", "segments_median", "segments_wide", "true_peak", "apply_f32")


def med(v):
    return float(np.median(np.array(v)))


def median_hop_energy(torch, out, counts, streams=1024):
    """the median energy of the whole hops of the first `streams` streams, as the sink computes it"""
    x = out[:streams].double()
    m = ((x[:, :, 0] + x[:, :, 1]).float() * 0.5).double()
    q = torch.clamp(torch.floor(m * 32768.0 + 0.5), -32768.0, 32767.0)
    hops = q.shape[1] // H
    E = (q[:, : hops * H] ** 2).reshape(q.shape[0], hops, H).sum(dim=2)
    whole = torch.arange(hops, device=E.device)[None, :] < (counts[:streams, None] // H)
    return max(int(E[whole].median().item()), 1)


def batch_part(a, torch, _gen, mp3_amd):
    n, F = a.streams, a.frames
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_true_peak(True)
    dec.set_segments(True)
    P, S = dec._segments
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    SS = mp3_amd.packed_max_samples(HZ, F, 44100)
    out = torch.empty((n, SS, CH), dtype=torch.float32, device="cuda")
    scaled = torch.empty_like(out)
    wide = torch.empty((n, mp3_amd.packed_max_samples(HZ, F), CH), dtype=torch.float32, device="cuda")
    seg = torch.zeros((n, mp3_amd.segment_max(HZ, SS, P, S), 2), dtype=torch.int64, device="cuda")
    gain = torch.ones(n, dtype=torch.float32, device="cuda")
    tp = torch.zeros(n, dtype=torch.float32, device="cuda")
    dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos)
    dec.sync()
    wide[:, :SS] = out
    thr_med = median_hop_energy(torch, out, counts)
    thr_40 = mp3_amd.segment_threshold(HZ, -40.0)
    dec.reset()
    times = {k: [] for k in VARIANTS}
    stage = {k: {"resample": [], "segment": []} for k in VARIANTS}
    emitted = {}
    samples = 0
    per = max(1, a.steps // a.rounds)

    def step(k):
        if k == "decode_segments":
            dec.decode_segments(d_in, offs, sizes, F, seg=seg, counts=sc, infos=infos, stream=strm.cuda_stream)
        elif k in ("segments", "segments_median"):
            dec.segments(out, counts, seg=seg, seg_counts=sc, stream=strm.cuda_stream)
        elif k == "segments_wide":
            dec.segments(wide, counts, seg=seg, seg_counts=sc, stream=strm.cuda_stream)
        elif k == "true_peak":
            dec.true_peak(out, counts, tpeak=tp, stream=strm.cuda_stream)
        elif k == "apply_f32":
            dec.apply_gain(out, counts, gain, out=scaled, stream=strm.cuda_stream)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)

    for _ in range(a.rounds):
        for k in VARIANTS:
            if k in ("segments", "segments_median", "segments_wide", "decode_segments"):
                dec.set_segment_threshold(energy=[thr_med if k == "segments_median" else thr_40] * n)
            for i in range(a.warmup + per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(strm)
                step(k)
                e1.record(strm)
                e1.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
                    if k in ("packed", "decode_segments"):
                        stage[k]["resample"].append(dec.resample_time_us())
                    if k in ("decode_segments", "segments", "segments_median", "segments_wide"):
                        stage[k]["segment"].append(dec.segment_time_us())
            print("%s: %.0f us" % (k, med(times[k])), file=sys.stderr, flush=True)
            if k == "packed":
                samples = int(counts.cpu().numpy().astype(np.int64).sum())
            if k in ("segments", "segments_median"):
                emitted[k] = int(sc.cpu().numpy().astype(np.int64).sum())
    res = {"shape": [n, F], "format": [HZ, CH], "steps": len(times["packed"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us", "samples_per_call": samples,
           "pause_speech_hops": [P, S], "threshold_minus40": thr_40, "threshold_median": thr_med,
           "segments_per_call": emitted}
    base = med(times["packed"])
    for k in VARIANTS:
        t = np.array(times[k])
        r = res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                      "step_over_packed": float(np.median(t) / base)}
        if stage[k]["resample"]:
            r["resample_stage_median"] = med(stage[k]["resample"])
        if k in ("apply_f32", "true_peak"):
            byts = samples * CH * (8 if k == "apply_f32" else 4)
            r.update({"bytes_per_s": byts / (np.median(t) * 1e-6),
                      "share_of_measured_hbm": byts / (np.median(t) * 1e-6) / HBM_MEASURED})
        if stage[k]["segment"]:
            st = med(stage[k]["segment"])
            byts = samples * CH * 4
            r.update({"segment_stage_median": st, "segment_stage_min": float(np.min(stage[k]["segment"])),
                      "segment_stage_max": float(np.max(stage[k]["segment"])),
                      "segment_stage_share_of_step": st / float(np.median(t)),
                      "segment_stage_ns_per_sample": st * 1e3 / max(samples, 1),
                      "segment_stage_read_bytes_per_s": byts / (st * 1e-6),
                      "segment_stage_share_of_measured_hbm": byts / (st * 1e-6) / HBM_MEASURED})
            if "resample_stage_median" in r:
                r["segment_stage_over_resample_stage"] = st / r["resample_stage_median"]
    # the floor: the stage's read at the rate apply_gain moves its bytes (it reads and writes as many)
    floor = samples * CH * 4 / res["apply_f32"]["bytes_per_s"] * 1e6
    res["read_floor_at_apply_gain_rate"] = floor
    for k in ("segments", "segments_median", "segments_wide", "decode_segments"):
        res[k]["segment_stage_over_read_floor"] = res[k]["segment_stage_median"] / floor
        res[k]["segment_stage_over_true_peak"] = res[k]["segment_stage_median"] / res["true_peak"]["step_median"]
    return res


def long_part(a, torch, _gen, mp3_amd):
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_segments(True)
    P, S = dec._segments
    bound = mp3_amd.long_packed_bound(data, HZ)
    out = torch.empty((bound, CH), dtype=torch.float32, device="cuda")
    seg = torch.zeros((1, mp3_amd.segment_max(HZ, bound, P, S), 2), dtype=torch.int64, device="cuda")
    sc = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_long, t_call, t_stage = [], [], []
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
        dec.segments(out[None], cnt, seg=seg, seg_counts=sc, flush=True)
        dec.sync()
        t3 = time.perf_counter()
        if i >= a.warmup:
            t_long.append((t1 - t0) * 1e6)
            t_call.append((t3 - t2) * 1e6)
            t_stage.append(dec.segment_time_us())
    return {"frames": a.long_frames, "out_samples": n, "hops": -(-n // H), "segments": int(sc.cpu()[0]),
            "decode_long_packed_call_median": med(t_long), "segments_call_median": med(t_call),
            "segments_stage_median": med(t_stage), "segments_call_over_decode_long_packed": med(t_call) / med(t_long),
            "segments_stage_ns_per_sample": med(t_stage) * 1e3 / max(n, 1),
            "segments_stage_read_bytes_per_s": n * CH * 4 / (med(t_stage) * 1e-6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
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
