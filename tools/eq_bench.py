#!/usr/bin/env python3
"""Time the equaliser sink against the packed 48 kHz stereo decode, the
resample stage and the loudness stage.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed             decode_packed, 44.1 -> 48 kHz stereo (the yardstick)
  packed_eq1 .. 10   decode_packed, then eq on its out and counts, with the
                     first K = 1, 2, 5, 10 bands of the graphic curve
  decode_equalized   decode_equalized at K = 10: the same through handle-owned
                     samples
  loudness           loudness alone on the packed out: a two-section cascade in
                     the same arithmetic without a store
and the device time of the equaliser stage (eq_time_us) next to the resample
stage (resample_time_us) and the loudness stage (loudness_time_us).  The
variants alternate in rounds inside one process; every step is timed by device
events on the call's stream.  No call flushes.  Work of the stage per sample,
channel and section, from its code: 5 FMA + 1 product in double, twice (the
zero-state pass, the true pass): 22 FLOP; bytes per sample and channel: 4 read
by k_eq_local (not for a stream's last tile), 4 read and 4 written by
k_eq_apply.

Then one long stream: eq on the device output of decode_long_packed (20 000
generated frames to 48 kHz stereo, as tools/limiter_bench.py), n = 1, at
K = 2 and 10, by the host clock around the synchronous calls, against that
call's own time.  Prints one JSON line (and writes it to --out).

  python tools/eq_bench.py --out profiles/eq.json
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
FP64_PEAK = 78.6e12  # the FP64 vector rate DESIGN.md section 4e uses
FLOP_PER_SAMPLE_CHANNEL_SECTION = 2 * 11
HZ, CH = 48000, 2
KS = (1, 2, 5, 10)
VARIANTS = ("packed",) + tuple("packed_eq%d" % k for k in KS) + ("decode_equalized", "loudness")


def med(v):
    return float(np.median(np.array(v)))


def graphic(k):
    """the first k octave bands from 31.25 Hz, alternating +-12 dB, Q 1.41; preamp -6 dB"""
    return [(0, 31.25 * 2 ** i, 12.0 if i % 2 == 0 else -12.0, 1.41) for i in range(k)], -6.0


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
    oc = torch.zeros(n, dtype=torch.int32, device="cuda")
    S = mp3_amd.packed_max_samples(HZ, F, 44100)
    out = torch.empty((n, S, CH), dtype=torch.float32, device="cuda")
    eqo = torch.empty_like(out)
    blocks = torch.empty((n, mp3_amd.loud_max_blocks(HZ, F, 44100)), dtype=torch.float32, device="cuda")
    bc = torch.zeros(n, dtype=torch.int32, device="cuda")
    peak = torch.zeros(n, dtype=torch.float32, device="cuda")
    times = {k: [] for k in VARIANTS}
    stage = {k: {"resample": [], "eq": [], "loudness": []} for k in VARIANTS}
    fed = {}
    per = max(1, a.steps // a.rounds)

    def step(k):
        if k == "decode_equalized":
            dec.decode_equalized(d_in, offs, sizes, F, out=eqo, counts=oc, infos=infos, stream=strm.cuda_stream)
        elif k == "loudness":
            dec.loudness(out, counts, blocks=blocks, block_counts=bc, peak=peak, stream=strm.cuda_stream)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)
            if k != "packed":
                dec.eq(out, counts, out=eqo, out_counts=oc, stream=strm.cuda_stream)

    for _ in range(a.rounds):
        for k in VARIANTS:
            if k.startswith("packed_eq"):
                dec.set_eq(*graphic(int(k[len("packed_eq"):])))
            elif k == "decode_equalized":
                dec.set_eq(*graphic(10))
            for i in range(a.warmup + per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(strm)
                step(k)
                e1.record(strm)
                e1.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
                    if k != "loudness":
                        stage[k]["resample"].append(dec.resample_time_us())
                    if k == "loudness":
                        stage[k]["loudness"].append(dec.loudness_time_us())
                    elif k != "packed":
                        stage[k]["eq"].append(dec.eq_time_us())
            print("%s: %.0f us" % (k, med(times[k])), file=sys.stderr, flush=True)
            if k == "packed":
                fed["samples"] = int(counts.cpu().numpy().astype(np.int64).sum())
    samples = fed["samples"]  # steady state: every call feeds a call's inputs' worth of samples
    res = {"shape": [n, F], "format": [HZ, CH], "steps": len(times["packed"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us", "samples_per_call": samples,
           "curve": "graphic: octave bands from 31.25 Hz, +-12 dB, Q 1.41, preamp -6 dB"}
    base = med(times["packed"])
    for k in VARIANTS:
        t = np.array(times[k])
        r = res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                      "step_over_packed": float(np.median(t) / base)}
        if stage[k]["resample"]:
            r["resample_stage_median"] = med(stage[k]["resample"])
        if stage[k]["loudness"]:
            r["loudness_stage_median"] = med(stage[k]["loudness"])
        if stage[k]["eq"]:
            K = 10 if k == "decode_equalized" else int(k[len("packed_eq"):])
            et = med(stage[k]["eq"])
            flop = samples * CH * K * FLOP_PER_SAMPLE_CHANNEL_SECTION
            byts = samples * CH * 12
            r.update({"sections": K, "eq_stage_median": et, "eq_stage_min": float(np.min(stage[k]["eq"])),
                      "eq_stage_share_of_step": et / float(np.median(t)),
                      "eq_stage_ns_per_sample_frame": et * 1e3 / max(samples, 1),
                      "eq_stage_over_resample_stage": et / r["resample_stage_median"],
                      "eq_stage_fp64_flop_per_s": flop / (et * 1e-6),
                      "eq_stage_share_of_fp64_peak": flop / (et * 1e-6) / FP64_PEAK,
                      "eq_stage_bytes_per_s": byts / (et * 1e-6),
                      "eq_stage_share_of_measured_hbm": byts / (et * 1e-6) / HBM_MEASURED})
    ld = res["loudness"]["loudness_stage_median"]
    for k in VARIANTS:
        if "eq_stage_median" in res[k]:
            res[k]["eq_stage_over_loudness_stage"] = res[k]["eq_stage_median"] / ld
    ts = np.array([res["packed_eq%d" % k]["eq_stage_median"] for k in KS])
    slope, icept = np.polyfit(np.array(KS, np.float64), ts, 1)
    res["eq_stage_per_section"] = {"slope_us": float(slope), "intercept_us": float(icept),
                                   "slope_ns_per_sample_frame": float(slope) * 1e3 / max(samples, 1)}
    res["decode_equalized"]["step_over_packed_eq10"] = (res["decode_equalized"]["step_median"]
                                                         / res["packed_eq10"]["step_median"])
    return res


def long_part(a, torch, _gen, mp3_amd):
    data, _ = _gen.stream(_gen.C3, 3_000_017, a.long_frames)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dec = mp3_amd.BatchDecoder(1024, 32 + 11)
    dec.set_timing(True)
    dec.set_output(HZ, CH)
    bound = mp3_amd.long_packed_bound(data, HZ)
    out = torch.empty((bound, CH), dtype=torch.float32, device="cuda")
    eqo = torch.empty((1, bound, CH), dtype=torch.float32, device="cuda")
    oc = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {"frames": a.long_frames}
    for K in (2, 10):
        dec.set_eq(*graphic(K))
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
            dec.eq(out[None], cnt, out=eqo, out_counts=oc, flush=True)
            dec.sync()
            t3 = time.perf_counter()
            if i >= a.warmup:
                t_long.append((t1 - t0) * 1e6)
                t_call.append((t3 - t2) * 1e6)
                t_stage.append(dec.eq_time_us())
        assert int(oc.cpu()[0]) == n
        res["out_samples"] = n
        res["decode_long_packed_call_median"] = med(t_long)
        res["eq%d" % K] = {"eq_call_median": med(t_call), "eq_stage_median": med(t_stage),
                           "eq_call_over_decode_long_packed": med(t_call) / med(t_long),
                           "eq_stage_ns_per_sample_frame": med(t_stage) * 1e3 / max(n, 1),
                           "eq_stage_bytes_per_s": n * CH * 12 / (med(t_stage) * 1e-6)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
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
