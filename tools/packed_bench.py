#!/usr/bin/env python3
"""Time the packed uniform-rate PCM sink against the plain float32 decode.

At one shape (default the C3 shape, 65 536 streams x 32 frames, 44.1 kHz
joint stereo) and with device pointers throughout, measures per step
  plain      BatchDecoder.decode(f32=True) into the caller's rows
  48k_stereo decode_packed, 44.1 -> 48 kHz stereo
  16k_mono   decode_packed, 44.1 -> 16 kHz mono
and, for the packed variants, the resample stage's own device time
(resample_time_us).  The variants alternate in rounds inside one process;
every step is timed by device events on the call's stream.  FLOP and bytes of
the stage are computed from the shapes: 2 T flop per output sample and
channel; the audio samples of the rows read once, the packed samples written
once.  Prints one JSON line (and writes it to --out).

  python tools/packed_bench.py --out profiles/packed_sink.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _gen
    import mp3_amd

    assert torch.cuda.is_available(), "needs an MI355X"
    n, F = a.streams, a.frames
    buf, offs, sizes = _gen.batch(_gen.C3, 3_000_017, n, F, threads=16)
    d_in = torch.from_numpy(buf).cuda()
    dec = mp3_amd.BatchDecoder(n, F)
    dec.set_timing(True)
    strm = torch.cuda.Stream()
    infos = torch.zeros((n, F, 6), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    rows = torch.empty((n, F, 2304), dtype=torch.float32, device="cuda")
    variants = {"plain": None, "48k_stereo": (48000, 2), "16k_mono": (16000, 1)}
    outs = {k: torch.empty((n, mp3_amd.packed_max_samples(v[0], F, 44100), v[1]), dtype=torch.float32, device="cuda")
            for k, v in variants.items() if v}
    times = {k: [] for k in variants}
    stage = {k: [] for k in variants if variants[k]}
    per = max(1, a.steps // a.rounds)
    emitted = {}

    def step(k):
        if variants[k] is None:
            dec.decode(d_in, offs, sizes, F, pcm=rows, infos=infos, stream=strm.cuda_stream, f32=True)
        else:
            dec.decode_packed(d_in, offs, sizes, F, out=outs[k], counts=counts, infos=infos, stream=strm.cuda_stream)

    for _ in range(a.rounds):
        for k, fmt in variants.items():
            if fmt:
                dec.set_output(*fmt)
            for i in range(a.warmup + per):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(strm)
                step(k)
                e1.record(strm)
                e1.synchronize()
                if i >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
                    if fmt:
                        stage[k].append(dec.resample_time_us())
            if fmt:
                emitted[k] = int(counts.cpu().numpy().astype(np.int64).sum())
    res = {"shape": [n, F], "steps": len(times["plain"]), "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "us"}
    frames_audio = int((infos.cpu().numpy()[..., 5] > 0).sum())
    for k, fmt in variants.items():
        t = np.array(times[k])
        r = {"step_median": float(np.median(t)), "step_min": float(t.min()), "step_max": float(t.max())}
        if fmt:
            L, M, taps = mp3_amd.resample_filter(44100, fmt[0])
            T = taps.shape[1]
            # steady state (no flush): a call emits its inputs' worth of outputs
            out_est = frames_audio * 1152 * L / M
            st = np.array(stage[k])
            flop = 2.0 * T * out_est * fmt[1]
            byts = frames_audio * 1152 * 2 * 4 + out_est * fmt[1] * 4
            r.update({"stage_median": float(np.median(st)), "stage_min": float(st.min()), "taps": T,
                      "stage_flop": flop, "stage_bytes": byts,
                      "stage_flop_per_s": flop / (np.median(st) * 1e-6),
                      "stage_bytes_per_s": byts / (np.median(st) * 1e-6),
                      "stage_share_of_fp32_vector_peak": flop / (np.median(st) * 1e-6) / FP32_VECTOR_PEAK,
                      "stage_share_of_measured_hbm": byts / (np.median(st) * 1e-6) / HBM_MEASURED,
                      "step_over_plain": float(np.median(t) / np.median(times["plain"]))})
            r["last_call_samples"] = emitted[k]
        res[k] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
