#!/usr/bin/env python3
"""Time the pitch sink against the packed decode, the resample stage and the
tempo sink's stretch stage.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz joint
stereo) and with device pointers throughout, per output format (16 kHz mono,
48 kHz stereo) one handle and one batch measure per step
  packed        decode_packed to the format (the yardstick)
  decode_pitch  decode_pitch: the same into handle-owned samples, then the stage
  pitch         the stage alone on the packed out (fmin 60, fmax 500, 0.15)
  stretch       the tempo sink's stage alone on the same samples at tempo 9/10:
                the nearest kernel, the same packed dot products
and the device time of the pitch stage (pitch_time_us) next to the resample
stage (resample_time_us) and the stretch stage (stretch_time_us).  The variants
alternate in rounds inside one process; every step is timed by device events on
the call's stream.  No call flushes.

The floor is the issue rate of the stage's packed dot products alone: a frame
costs 16 * ceil(H / 4) * nt / 64 wave-level v_dot2 (nt = 2 (T / 8 + 1) threads
own lags, mp3d_pitch.h), four cycles each on one of 1024 SIMDs at --clock-mhz
(default 2100, the sustained clock of profiles/r06_clk.json under load).

Then one long stream: the stage on the device output of decode_long_packed
(20 000 generated frames to 48 kHz stereo), n = 1, flushed, by the host clock
around the synchronous calls.  Prints one JSON line (and writes it to --out).

  python tools/pitch_bench.py --out profiles/pitch.json
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

FMIN, FMAX, THR = 60, 500, 0.15
VARIANTS = ("packed", "decode_pitch", "pitch", "stretch")
SIMDS = 256 * 4


def med(v):
    return float(np.median(np.array(v)))


def dot2_per_frame(hz):
    """wave-level packed dot products of one frame (mp3d_pitch.h)"""
    H, T = (hz + 50) // 100, hz // FMIN + 1
    nt = 2 * (T // 8 + 1)
    return 16 * -(-H // 4) * nt / 64.0


def batch_part(a, torch, _gen, mp3_amd, d_in, offs, sizes, hz, ch):
    n, F = a.streams, a.frames
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    dec.set_output(hz, ch)
    dec.set_stretch(True)
    dec.set_tempo([9] * n, [10] * n)
    dec.set_pitch(True, FMIN, FMAX, THR)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    pc = torch.zeros(n, dtype=torch.int32, device="cuda")
    oc = torch.zeros(n, dtype=torch.int32, device="cuda")
    SS = mp3_amd.packed_max_samples(hz, F, 44100)
    out = torch.empty((n, SS, ch), dtype=torch.float32, device="cuda")
    rec = torch.zeros((n, mp3_amd.pitch_max_frames(hz, mp3_amd.packed_max_samples(hz, F), FMIN), 4),
                      dtype=torch.int32, device="cuda")
    so = torch.empty((n, mp3_amd.stretch_max_samples(hz, SS, 9, 10), ch), dtype=torch.float32, device="cuda")
    dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos)
    dec.sync()
    dec.reset()
    times = {k: [] for k in VARIANTS}
    stage = {k: [] for k in VARIANTS}
    rs = []
    frames = samples = voiced = 0
    per = max(1, a.steps // a.rounds)

    def step(k):
        if k == "decode_pitch":
            dec.decode_pitch(d_in, offs, sizes, F, out=rec, counts=pc, infos=infos, stream=strm.cuda_stream)
        elif k == "pitch":
            dec.pitch(out, counts, out=rec, out_counts=pc, stream=strm.cuda_stream)
        elif k == "stretch":
            dec.stretch(out, counts, out=so, out_counts=oc, stream=strm.cuda_stream)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)

    for _ in range(a.rounds):
        for k in VARIANTS:
            for i in range(a.warmup + per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(strm)
                step(k)
                e1.record(strm)
                e1.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
                    if k in ("packed", "decode_pitch"):
                        rs.append(dec.resample_time_us())
                    if k in ("decode_pitch", "pitch"):
                        stage[k].append(dec.pitch_time_us())
                    if k == "stretch":
                        stage[k].append(dec.stretch_time_us())
            print("%d Hz x %d %s: %.0f us" % (hz, ch, k, med(times[k])), file=sys.stderr, flush=True)
            if k == "packed":
                samples = int(counts.cpu().numpy().astype(np.int64).sum())
            if k == "pitch":
                frames = int(pc.cpu().numpy().astype(np.int64).sum())
                voiced = float((rec[:256, :, 2] > 0).float().mean().item())
    base = med(times["packed"])
    res = {"format": [hz, ch], "samples_per_call": samples, "frames_per_pitch_call": frames,
           "voiced_share_first_256_rows": voiced, "resample_stage_median": med(rs)}
    for k in VARIANTS:
        t = np.array(times[k])
        res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                  "step_over_packed": float(np.median(t) / base)}
        if stage[k]:
            res[k]["stage_median"] = med(stage[k])
            res[k]["stage_min"], res[k]["stage_max"] = float(np.min(stage[k])), float(np.max(stage[k]))
    dpf = dot2_per_frame(hz)
    floor = frames * dpf * 4 / SIMDS / (a.clock_mhz * 1e6) * 1e6
    st = res["pitch"]["stage_median"]
    res.update({"wave_dot2_per_frame": dpf, "dot2_floor_us": floor, "clock_mhz_assumed": a.clock_mhz,
                "pitch_stage_over_dot2_floor": st / floor if floor else None,
                "pitch_stage_over_resample_stage": st / res["resample_stage_median"],
                "pitch_stage_over_stretch_stage": st / res["stretch"]["stage_median"],
                "pitch_stage_us_per_frame": st / max(frames, 1)})
    return res


def long_part(a, torch, _gen, mp3_amd):
    hz, ch = 48000, 2
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(hz, ch)
    dec.set_pitch(True, FMIN, FMAX, THR)
    bound = mp3_amd.long_packed_bound(data, hz)
    out = torch.empty((bound, ch), dtype=torch.float32, device="cuda")
    rec = torch.zeros((1, mp3_amd.pitch_max_frames(hz, bound, FMIN), 4), dtype=torch.int32, device="cuda")
    pc = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_long, t_call, t_stage = [], [], []
    n = 0
    for i in range(a.warmup + a.long_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = dec.decode_long_packed(d_in, hz, ch, segment_frames=32, out=out, gapless=True)
        t1 = time.perf_counter()
        n = int(len(r[0]))
        cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dec.pitch(out[None], cnt, out=rec, out_counts=pc, flush=True)
        dec.sync()
        t3 = time.perf_counter()
        if i >= a.warmup:
            t_long.append((t1 - t0) * 1e6)
            t_call.append((t3 - t2) * 1e6)
            t_stage.append(dec.pitch_time_us())
    k = int(pc.cpu()[0])
    return {"frames": a.long_frames, "out_samples": n, "pitch_frames": k,
            "decode_long_packed_call_median": med(t_long), "pitch_call_median": med(t_call),
            "pitch_stage_median": med(t_stage), "pitch_call_over_decode_long_packed": med(t_call) / med(t_long),
            "pitch_stage_us_per_frame": med(t_stage) / max(k, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--long-frames", type=int, default=20000)
    ap.add_argument("--long-steps", type=int, default=5)
    ap.add_argument("--clock-mhz", type=float, default=2100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, a.streams, a.frames, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    res = {"shape": [a.streams, a.frames], "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us", "limits": [FMIN, FMAX, THR]}
    for hz, ch in ((16000, 1), (48000, 2)):
        res["%d_%d" % (hz, ch)] = batch_part(a, torch, _gen, mp3_amd, d_in, offs, sizes, hz, ch)
        torch.cuda.empty_cache()
    res["long"] = long_part(a, torch, _gen, mp3_amd)
    print(json.dumps(res))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
