#!/usr/bin/env python3
"""Time the true-peak tap and the gain kernels against the packed 48 kHz
stereo decode and the loudness stage.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed           decode_packed, 44.1 -> 48 kHz stereo (the yardstick)
  packed_tap       decode_packed, then true_peak on its out and counts
  decode_loudness  decode_loudness (the samples stay in the handle)
  decode_measure   decode_measure: the same plus the true-peak stage
  apply_f32        apply_gain alone on the packed out, float32 to float32
  apply_i16        apply_gain alone, float32 to int16
and the device time of the true-peak stage (true_peak_time_us) next to the
loudness stage (loudness_time_us) of those steps.  The variants alternate in
rounds inside one process; every step is timed by device events on the call's
stream.  Work of the true-peak stage per sample and channel, from its code:
3 phases x 12 FMA = 72 FLOP in float32 against 4 bytes read once; apply_gain
reads 4 bytes and writes 4 or 2 per element.

Then one long stream: the tap on the device output of decode_long_packed
(20 000 generated frames to 48 kHz stereo, as tools/loudness_bench.py), n = 1,
by the host clock around the synchronous calls, against that call's own time.
Prints one JSON line (and writes it to --out).

  python tools/normalize_bench.py --out profiles/normalize.json
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
FLOP_PER_SAMPLE_CHANNEL = 2 * 3 * 12
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
    dec.set_true_peak(True)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty((n, mp3_amd.packed_max_samples(HZ, F, 44100), CH), dtype=torch.float32, device="cuda")
    scaled = torch.empty_like(out)
    scaled16 = torch.empty(out.shape, dtype=torch.int16, device="cuda")
    blocks = torch.empty((n, mp3_amd.loud_max_blocks(HZ, F, 44100)), dtype=torch.float32, device="cuda")
    bc = torch.zeros(n, dtype=torch.int32, device="cuda")
    peak = torch.zeros(n, dtype=torch.float32, device="cuda")
    tpeak = torch.zeros(n, dtype=torch.float32, device="cuda")
    gain = torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
    variants = ("packed", "packed_tap", "decode_loudness", "decode_measure", "apply_f32", "apply_i16")
    times = {k: [] for k in variants}
    stage = {k: {"resample": [], "loudness": [], "true_peak": []} for k in variants}
    fed = {}
    per = max(1, a.steps // a.rounds)

    def step(k):
        if k == "decode_loudness":
            dec.decode_loudness(d_in, offs, sizes, F, blocks=blocks, counts=bc, peak=peak, infos=infos,
                                stream=strm.cuda_stream)
        elif k == "decode_measure":
            dec.decode_measure(d_in, offs, sizes, F, blocks=blocks, counts=bc, peak=peak, tpeak=tpeak, infos=infos,
                               stream=strm.cuda_stream)
        elif k == "apply_f32":
            dec.apply_gain(out, counts, gain, out=scaled, stream=strm.cuda_stream)
        elif k == "apply_i16":
            dec.apply_gain(out, counts, gain, out=scaled16, f32=False, stream=strm.cuda_stream)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)
            if k == "packed_tap":
                dec.true_peak(out, counts, tpeak=tpeak, stream=strm.cuda_stream)

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
                    if not k.startswith("apply"):
                        stage[k]["resample"].append(dec.resample_time_us())
                    if k in ("decode_loudness", "decode_measure"):
                        stage[k]["loudness"].append(dec.loudness_time_us())
                    if k in ("packed_tap", "decode_measure"):
                        stage[k]["true_peak"].append(dec.true_peak_time_us())
            print("%s: %.0f us" % (k, med(times[k])), file=sys.stderr, flush=True)
            if k == "packed_tap":
                fed["samples"] = int(counts.cpu().numpy().astype(np.int64).sum())
    res = {"shape": [n, F], "format": [HZ, CH], "steps": len(times["packed"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us", "samples_per_call": fed["samples"]}
    base = med(times["packed"])
    samples = fed["samples"]  # steady state: every call feeds a call's inputs' worth of samples
    for k in variants:
        t = np.array(times[k])
        r = res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                      "step_over_packed": float(np.median(t) / base)}
        if k.startswith("apply"):
            byts = samples * CH * (4 + (4 if k == "apply_f32" else 2))
            r.update({"bytes_per_s": byts / (np.median(t) * 1e-6),
                      "share_of_measured_hbm": byts / (np.median(t) * 1e-6) / HBM_MEASURED})
            continue
        r["resample_stage_median"] = med(stage[k]["resample"])
        if stage[k]["loudness"]:
            r["loudness_stage_median"] = med(stage[k]["loudness"])
        if stage[k]["true_peak"]:
            tp = med(stage[k]["true_peak"])
            flop, byts = samples * CH * FLOP_PER_SAMPLE_CHANNEL, samples * CH * 4
            r.update({"true_peak_stage_median": tp, "true_peak_stage_min": float(np.min(stage[k]["true_peak"])),
                      "true_peak_stage_over_resample_stage": tp / r["resample_stage_median"],
                      "true_peak_stage_share_of_step": tp / float(np.median(t)),
                      "true_peak_stage_ns_per_sample": tp * 1e3 / max(samples, 1),
                      "true_peak_stage_fp32_flop_per_s": flop / (tp * 1e-6),
                      "true_peak_stage_bytes_per_s": byts / (tp * 1e-6),
                      "true_peak_stage_share_of_measured_hbm": byts / (tp * 1e-6) / HBM_MEASURED})
    m, l = res["decode_measure"], res["decode_loudness"]
    m["step_over_decode_loudness"] = m["step_median"] / l["step_median"]
    m["true_peak_stage_over_loudness_stage"] = m["true_peak_stage_median"] / m["loudness_stage_median"]
    return res


def long_part(a, torch, _gen, mp3_amd):
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_loudness(True)
    dec.set_true_peak(True)
    out = torch.empty((mp3_amd.long_packed_bound(data, HZ), CH), dtype=torch.float32, device="cuda")
    H = (HZ + 5) // 10
    blocks = torch.empty((1, out.shape[0] // H + 1), dtype=torch.float32, device="cuda")
    bc = torch.zeros(1, dtype=torch.int32, device="cuda")
    peak = torch.zeros(1, dtype=torch.float32, device="cuda")
    tpeak = torch.zeros(1, dtype=torch.float32, device="cuda")
    t_long, t_tap, t_stage, t_ld = [], [], [], []
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
        dec.true_peak(out[None], cnt, tpeak=tpeak, flush=True)
        dec.sync()
        t3 = time.perf_counter()
        dec.loudness(out[None], cnt, blocks=blocks, block_counts=bc, peak=peak, flush=True)
        dec.sync()
        if i >= a.warmup:
            t_long.append((t1 - t0) * 1e6)
            t_tap.append((t3 - t2) * 1e6)
            t_stage.append(dec.true_peak_time_us())
            t_ld.append(dec.loudness_time_us())
    return {"frames": a.long_frames, "out_samples": n, "tpeak": float(tpeak.cpu()[0]), "peak": float(peak.cpu()[0]),
            "decode_long_packed_call_median": med(t_long), "tap_call_median": med(t_tap),
            "tap_stage_median": med(t_stage), "loudness_stage_median": med(t_ld),
            "tap_call_over_decode_long_packed": med(t_tap) / med(t_long),
            "tap_stage_over_loudness_stage": med(t_stage) / med(t_ld),
            "tap_stage_ns_per_sample": med(t_stage) * 1e3 / max(n, 1),
            "tap_stage_bytes_per_s": n * CH * 4 / (med(t_stage) * 1e-6)}


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
