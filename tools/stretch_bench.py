#!/usr/bin/env python3
"""Time the tempo sink (the WSOLA stretch stage) against the packed 48 kHz
stereo decode it runs on.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed        decode_packed, 44.1 -> 48 kHz stereo (the yardstick)
  stretch N/D   decode_packed, then stretch on its out and counts with every
                stream at tempo N/D (1/2, 9/10, 2/1), not flushed: the streams
                go on from call to call, so every call emits a call's worth
and the device time of the stretch stage (stretch_time_us) next to the
resample stage (resample_time_us) of the same step.  Every step is timed by
device events on the call's stream.  Work of the stage per emitted block of H
= 480 samples, from its code: 481 candidates x 240 sample pairs, one packed
int16 subtract and one packed int16 dot product each, on 1440 staged int16.

Then one long stream: the stage with n_streams = 1 on the device output of
decode_long_packed (20 000 generated frames to 48 kHz stereo), flushed, by the
host clock around the synchronous calls, against that call's own time.  One
stream is a chain of blocks, so this runs on one compute unit.
Prints one JSON line (and writes it to --out).

  python tools/stretch_bench.py --out profiles/stretch.json
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

HZ, CH = 48000, 2
TEMPOS = [(1, 2), (9, 10), (2, 1)]


def med(v):
    return float(np.median(np.array(v)))


def batch_part(a, torch, _gen, mp3_amd):
    n, F = a.streams, a.frames
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_stretch(True)
    strm = torch.cuda.Stream()
    S = mp3_amd.packed_max_samples(HZ, F, 44100)
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty((n, S, CH), dtype=torch.float32, device="cuda")
    sout = torch.empty((n, mp3_amd.stretch_max_samples(HZ, S, 1, 2), CH), dtype=torch.float32, device="cuda")
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = {"shape": [n, F], "format": [HZ, CH], "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "unit": "us"}

    def run(tempo):
        if tempo:
            dec.set_tempo([tempo[0]] * n, [tempo[1]] * n)
        t, rs, st = [], [], []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(strm)
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)
            if tempo:
                dec.stretch(out, counts, out=sout, out_counts=sc, stream=strm.cuda_stream)
            e1.record(strm)
            e1.synchronize()
            if i >= a.warmup:
                t.append(e0.elapsed_time(e1) * 1e3)
                rs.append(dec.resample_time_us())
                if tempo:
                    st.append(dec.stretch_time_us())
        return t, rs, st

    t, rs, _ = run(None)
    base = med(t)
    res["packed"] = {"step_median": base, "step_min": float(np.min(t)), "resample_stage_median": med(rs)}
    res["samples_per_call"] = int(counts.cpu().numpy().astype(np.int64).sum())
    print("packed: %.0f us" % base, file=sys.stderr, flush=True)
    for tempo in TEMPOS:
        t, rs, st = run(tempo)
        emitted = int(sc.cpu().numpy().astype(np.int64).sum())
        assert (sc.cpu().numpy() >= 0).all()
        res["stretch %d/%d" % tempo] = {
            "step_median": med(t), "step_over_packed": med(t) / base, "resample_stage_median": med(rs),
            "stretch_stage_median": med(st), "stretch_stage_min": float(np.min(st)),
            "stretch_stage_over_packed_step": med(st) / base, "stretch_stage_over_resample_stage": med(st) / med(rs),
            "samples_emitted_per_call": emitted, "stretch_stage_ns_per_emitted_sample": med(st) * 1e3 / max(emitted, 1)}
        print("stretch %d/%d: stage %.0f us" % (tempo + (med(st),)), file=sys.stderr, flush=True)
    return res


def long_part(a, torch, _gen, mp3_amd):
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    dec.set_stretch(True)
    bound = mp3_amd.long_packed_bound(data, HZ)
    out = torch.empty((bound, CH), dtype=torch.float32, device="cuda")
    sout = torch.empty((1, mp3_amd.stretch_max_samples(HZ, bound, 1, 2), CH), dtype=torch.float32, device="cuda")
    sc = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_long = []
    for i in range(a.warmup + a.long_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = dec.decode_long_packed(d_in, HZ, CH, segment_frames=32, out=out, gapless=True)
        t_long.append((time.perf_counter() - t0) * 1e6)
    n = int(len(r[0]))
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    res = {"frames": a.long_frames, "in_samples": n, "decode_long_packed_call_median": med(t_long[a.warmup:])}
    for tempo in TEMPOS:
        dec.set_tempo(*tempo)
        t_call, t_stage = [], []
        for i in range(a.warmup + a.long_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.stretch(out[None], cnt, out=sout, out_counts=sc, flush=True)
            dec.sync()
            if i >= a.warmup:
                t_call.append((time.perf_counter() - t0) * 1e6)
                t_stage.append(dec.stretch_time_us())
        m = int(sc.cpu()[0])
        assert m == -(-n * tempo[1] // tempo[0])
        res["stretch %d/%d" % tempo] = {
            "out_samples": m, "call_median": med(t_call), "stage_median": med(t_stage),
            "stage_over_decode_long_packed": med(t_stage) / res["decode_long_packed_call_median"],
            "stage_us_per_block": med(t_stage) / max(1, -(-m // ((HZ + 50) // 100)))}
        print("long stretch %d/%d: stage %.0f us" % (tempo + (med(t_stage),)), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--long-frames", type=int, default=20000)
    ap.add_argument("--long-steps", type=int, default=3)
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
