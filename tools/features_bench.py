#!/usr/bin/env python3
"""Time the log-mel feature sink against the packed 16 kHz mono decode.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, one handle and one batch
measure per step
  packed_16k_mono  decode_packed, 44.1 -> 16 kHz mono
  features         decode_features, n_mels log-mel frames of the same samples
and the device time of the resample stage (resample_time_us) and of the
feature stage (feature_time_us) of the feature steps.  The variants alternate
in rounds inside one process; every step is timed by device events on the
call's stream.  FLOP of the feature stage per frame, from its code: the three
FFT passes, the unpack and power, and 2 flop per filter weight; bytes: the
samples read once, the features written once.  Prints one JSON line (and
writes it to --out).

  python tools/features_bench.py --out profiles/features.json
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FP32_VECTOR_PEAK = 157.3e12  # MI355X spec, FLOP/s
HBM_MEASURED = 6.29e12       # float4 copy, bytes/s

# real operations per frame: window 400; first radix-5 pass 40 butterflies of
# 72; second radix-5 pass 40 x (4 complex products of 6 + 72); radix-8 pass
# 25 x (7 complex products of 6 + 64 + 4 scalings of 2); unpack 201 x (8 +
# complex product 6 + 2) and power 201 x 3
FFT_FLOP = 400 + 40 * 72 + 40 * 96 + 25 * 114 + 201 * 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    n, F, nm = a.streams, a.frames, a.mels
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    dec.set_output(16000, 1)
    dec.set_features(nm, log10=True)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty((n, mp3_amd.packed_max_samples(16000, F, 44100), 1), dtype=torch.float32, device="cuda")
    feat = torch.empty((n, mp3_amd.feat_max_frames(F, 44100), nm), dtype=torch.float32, device="cuda")
    variants = ("packed_16k_mono", "features")
    times = {k: [] for k in variants}
    stage = {"resample": [], "features": []}
    per = max(1, a.steps // a.rounds)
    emitted = {}

    def step(k):
        if k == "features":
            dec.decode_features(d_in, offs, sizes, F, feat=feat, counts=counts, infos=infos, stream=strm.cuda_stream)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=out, counts=counts, infos=infos, stream=strm.cuda_stream)

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
                    if k == "features":
                        stage["resample"].append(dec.resample_time_us())
                        stage["features"].append(dec.feature_time_us())
            emitted[k] = int(counts.cpu().numpy().astype(np.int64).sum())
    res = {"shape": [n, F], "n_mels": nm, "steps": len(times["features"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us"}
    for k in variants:
        t = np.array(times[k])
        res[k] = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max()),
                  "last_call_emitted": emitted[k]}
    fb = mp3_amd.mel_filterbank(nm)
    frames_out = emitted["features"]          # steady state: a call's inputs' worth of frames
    samples_in = frames_out * 160
    ft, rs = np.array(stage["features"]), np.array(stage["resample"])
    flop = frames_out * (FFT_FLOP + 2.0 * int((fb != 0).sum()) + nm)
    byts = samples_in * 4 + frames_out * nm * 4
    sec = np.median(ft) * 1e-6
    res["features"].update({
        "step_over_packed": float(np.median(times["features"]) / np.median(times["packed_16k_mono"])),
        "stage_median": float(np.median(ft)), "stage_min": float(ft.min()),
        "resample_stage_median": float(np.median(rs)),
        "stage_over_resample_stage": float(np.median(ft) / np.median(rs)),
        "stage_ns_per_input_sample": float(np.median(ft) * 1e3 / max(samples_in, 1)),
        "stage_flop": flop, "stage_bytes": byts,
        "stage_flop_per_s": flop / sec, "stage_bytes_per_s": byts / sec,
        "stage_share_of_fp32_vector_peak": flop / sec / FP32_VECTOR_PEAK,
        "stage_share_of_measured_hbm": byts / sec / HBM_MEASURED})
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
