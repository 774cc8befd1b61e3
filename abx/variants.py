#!/usr/bin/env python3
"""Build k_synth phase-ablation variants (build_ab/NAME.so) for A/B timing only:
their output is wrong by construction.  Usage: python abx/variants.py"""
import sys

import stage

KERNELS = ["mp3d_demux.hip", "mp3d_huffman.hip", "mp3d_synth.hip", "mp3d_demux_dev.h", "mp3d_huffman_dev.h", "mp3d_internal.h"]


def variant(name, reps):
    srcs = {k: open("mp3_amd/csrc/" + k).read() for k in KERNELS}
    flags = [b for a, b in reps if a == "FLAGS"]
    reps = [(a, b) for a, b in reps if a != "FLAGS"]
    for a, b in reps:
        assert any(a in s for s in srcs.values()), (name, a)
        srcs = {k: s.replace(a, b) for k, s in srcs.items()}
    stage.build("/tmp/vars/" + name, "build_ab/%s.so" % name, srcs, extra=flags)


W4H = ("__global__ void __launch_bounds__(HUFF_BLOCK) k_huffman(",
       "__global__ void __launch_bounds__(HUFF_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) k_huffman(")
_QS = "            /* ---------------- phase Q: requantise + stereo -> LDS ---------- */"
_IS = "            /* ---------------- phase I: alias + IMDCT + overlap ------------ */"
_MS = "            /* ---------------- phase M: matrixing on the matrix cores ------- */"
_WS = "            /* ---------------- phase W: 512-tap window -> PCM --------------- */"


def _pr(n, marker):
    """s_setprio(n) just before a k_synth phase marker"""
    return (marker, "            __builtin_amdgcn_s_setprio(%d);\n%s" % (n, marker))


LID = "__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u))"
VARS = {
    # k_synth phase Q: channel 1 reuses channel 0's line-pair table word when both have the same block variant
    "LP1": [("""                for (int i = 0; i < 5; i++) {
                    const int l0 = 2 * lane + 128 * i;
                    const bool ok = i < 4 || lane < 32;
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const uint32_t tv2 = ok ? lpair[var[c]][l0 >> 1] : 0u;""",
             """                for (int i = 0; i < 5; i++) {
                    const int l0 = 2 * lane + 128 * i;
                    const bool ok = i < 4 || lane < 32;
                    uint32_t tvp[2];
                    tvp[0] = ok ? lpair[var[0]][l0 >> 1] : 0u;
                    if (var[1] == var[0]) tvp[1] = tvp[0];
                    else tvp[1] = ok ? lpair[var[1]][l0 >> 1] : 0u;
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const uint32_t tv2 = tvp[c];""")],
    # priority through phase Q = 2 (SP4), Q = 3 (SP6); Q 1 + M 2 (SP3); Q and I at 1 (SP5)
    "SP4": [_pr(2, _QS), _pr(0, _IS)],
    "SP6": [_pr(3, _QS), _pr(0, _IS)],
    "SP3": [_pr(1, _QS), _pr(0, _IS), _pr(2, _MS), _pr(0, _WS)],
    "SP5": [_pr(1, _QS), _pr(0, _MS)],
    # k_huffman: priority 1 while a round's segments stage into LDS, 0 for the decode (HP1)
    "HP1": [("                /* stage: each lane copies its own segment, 4 x 16 B in flight */",
             "                __builtin_amdgcn_s_setprio(1);\n                /* stage: each lane copies its own segment, 4 x 16 B in flight */"),
            ("                    /* big_values: region boundaries (ISO 2.4.2.7; FFmpeg clamp) */",
             "                    __builtin_amdgcn_s_setprio(0);\n                    /* big_values: region boundaries (ISO 2.4.2.7; FFmpeg clamp) */")],
    # k_huffman: priority 1 through the count1 loop (HP2) / through the big_values loop (HP3)
    "HP2": [("                    /* count1 quadruples until the part2_3 end; a quadruple that",
             "                    __builtin_amdgcn_s_setprio(1);\n                    /* count1 quadruples until the part2_3 end; a quadruple that"),
            ("                    const int nz_end = k;", "                    __builtin_amdgcn_s_setprio(0);\n                    const int nz_end = k;")],
    "HP3": [("                    for (; __ballot(k < bv2); k += 8) {",
             "                    __builtin_amdgcn_s_setprio(1);\n                    for (; __ballot(k < bv2); k += 8) {"),
            ("                    /* count1 quadruples until the part2_3 end; a quadruple that",
             "                    __builtin_amdgcn_s_setprio(0);\n                    /* count1 quadruples until the part2_3 end; a quadruple that")],
    # k_synth: priority 1 while a phase issues its LDS reads, 0 for its arithmetic (on top of phase Q at 1):
    # phase W's X reads (SW1), phase I's spectrum reads (SI1), phase M's S reads (SM1)
    "SW1": [("                float xa[18], xb[18];",
             "                __builtin_amdgcn_s_setprio(1);\n                float xa[18], xb[18];"),
            ("                /* output slots in pairs (t0, t1): lanes 0-31 hold L, lanes",
             "                __builtin_amdgcn_s_setprio(0);\n                /* output slots in pairs (t0, t1): lanes 0-31 hold L, lanes")],
    "SI1": [("                float x[18], up[8], dn[8];",
             "                __builtin_amdgcn_s_setprio(1);\n                float x[18], up[8], dn[8];"),
            ("                /* alias reduction (ISO 2.4.3.4): all 31 boundaries (long),",
             "                __builtin_amdgcn_s_setprio(0);\n                /* alias reduction (ISO 2.4.3.4): all 31 boundaries (long),")],
    "SM1": [("                float Be[3][4], Bo[3][4];",
             "                __builtin_amdgcn_s_setprio(1);\n                float Be[3][4], Bo[3][4];"),
            ("                f32x4 ce[3], co[3];",
             "                __builtin_amdgcn_s_setprio(0);\n                f32x4 ce[3], co[3];")],
    # k_synth: the next granule's prefetch issued at the start of phase Q (right after the current is[] words
    # are copied), phase Q reading the current meta words from a copy (PF1)
    "PF1": [("                    for (int i = 0; i < 5; i++) cis[c][i] = nis[c][i];",
             "                    for (int i = 0; i < 5; i++) cis[c][i] = nis[c][i];\n"
             "                const uint32_t cmeta = nmeta;\n"
             "                if (PF == 0 && (LSF ? f + 1 < f1 : (gr == 0 || f + 1 < f1))) prefetch(LSF ? 2 * f + 2 : 2 * f + gr + 1);"),
            ("                if (PF == 0 && (LSF ? f + 1 < f1 : (gr == 0 || f + 1 < f1))) prefetch(LSF ? 2 * f + 2 : 2 * f + gr + 1);\n                /* scatter",
             "                /* scatter"),
            ("((uint32_t *)&Wd.m[0])[lane] = nmeta;", "((uint32_t *)&Wd.m[0])[lane] = cmeta;"),
            ("readlane((int)nmeta, 10)", "readlane((int)cmeta, 10)"),
            ("readlane((int)nmeta, 11)", "readlane((int)cmeta, 11)"),
            ("readlane((int)nmeta, 12)", "readlane((int)cmeta, 12)"),
            ("readlane((int)nmeta, MW + 10)", "readlane((int)cmeta, MW + 10)"),
            ("readlane((int)nmeta, MW + 11)", "readlane((int)cmeta, MW + 11)"),
            ("readlane((int)nmeta, MW + 12)", "readlane((int)cmeta, MW + 12)"),
            ("__shfl((int)nmeta, cbase", "__shfl((int)cmeta, cbase")],
    # compiler scheduling knobs (all kernels): max-ILP / max-memory-clause strategies, latency-leaning metric
    # bias, LLVM's automatic wave-priority pass
    "SC1": [("FLAGS", "-mllvm"), ("FLAGS", "-amdgpu-sched-strategy=max-ilp")],
    "SC2": [("FLAGS", "-mllvm"), ("FLAGS", "-amdgpu-sched-strategy=max-memory-clause")],
    "SC3": [("FLAGS", "-mllvm"), ("FLAGS", "-amdgpu-schedule-metric-bias=0")],
    "SC4": [("FLAGS", "-mllvm"), ("FLAGS", "-amdgpu-set-wave-priority")],
    # k_synth streams per workgroup: 6 (two 6-wave workgroups per CU at 3 waves/SIMD; tables staged once per 6)
    "SW6": [("#define SYN_WAVES 4", "#define SYN_WAVES 6")],
    # phase-Q priority also on the synth-only (C2) entry (SPX)
    "SPX": [("            if (!SRC_XR) __builtin_amdgcn_s_setprio(1);", "            __builtin_amdgcn_s_setprio(1);"),
            ("            if (!SRC_XR) __builtin_amdgcn_s_setprio(0);", "            __builtin_amdgcn_s_setprio(0);")],
    # k_synth wave priority: raised through phase M (the MFMA chains issue ahead of other waves' VALU)
    "SP1": [("            /* ---------------- phase M: matrixing on the matrix cores ------- */",
             "            __builtin_amdgcn_s_setprio(2);\n            /* ---------------- phase M: matrixing on the matrix cores ------- */"),
            ("            /* ---------------- phase W: 512-tap window -> PCM --------------- */",
             "            __builtin_amdgcn_s_setprio(0);\n            /* ---------------- phase W: 512-tap window -> PCM --------------- */")],
    # k_synth wave priority: raised through phase Q (its loads and LDS table reads issue early)
    "SP2": [("            /* ---------------- phase Q: requantise + stereo -> LDS ---------- */",
             "            __builtin_amdgcn_s_setprio(1);\n            /* ---------------- phase Q: requantise + stereo -> LDS ---------- */"),
            ("            /* ---------------- phase I: alias + IMDCT + overlap ------------ */",
             "            __builtin_amdgcn_s_setprio(0);\n            /* ---------------- phase I: alias + IMDCT + overlap ------------ */")],
    # ranking key: part2_3_length / 16 (total bits: big_values + count1 work) instead of big_values
    "RK1": [("            bvk[j] = u < n_units ? (uint32_t)(sideu[u] >> 43) & 0x1FFu : 0u;",
             "            bvk[j] = u < n_units ? (uint32_t)(sideu[u] >> 56) & 0xFFu : 0u;")],
    # ranking key: big_values / 2 + part2_3_length / 32
    "RK2": [("            bvk[j] = u < n_units ? (uint32_t)(sideu[u] >> 43) & 0x1FFu : 0u;",
             "            bvk[j] = u < n_units ? (((uint32_t)(sideu[u] >> 43) & 0x1FFu) >> 1) + ((uint32_t)(sideu[u] >> 57) & 0x7Fu) : 0u;")],
    # r02 timing-only probes (wrong output): k_huffman with conflict-free window / LUT reads
    "HW0": [("    const uint32_t w0 = bits[w], w1 = bits[w + 1], w2 = bits[w + 2];",
             "    const uint32_t ln = " + LID + "; (void)w;\n    const uint32_t w0 = bits[ln], w1 = bits[ln + 64], w2 = bits[ln + 128];"),
            ("    const uint32_t w0 = bits[w], w1 = bits[w + 1];",
             "    const uint32_t ln = " + LID + "; (void)w;\n    const uint32_t w0 = bits[ln], w1 = bits[ln + 64];")],
    "LUT0": [("const uint32_t e1 = s_lut[i1];", "const uint32_t e1 = s_lut[(i1 & ~63u) + (uint32_t)lane];"),
             ("const uint32_t e = s_lut[i2];", "const uint32_t e = s_lut[(i2 & ~63u) + (uint32_t)lane_now()];")],
    # k_huffman row stores: suppressed (compute kept) / coalesced into one
    # contiguous 1 KB per wave instruction (output wrong; timing only)
    "NS1": [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
             "                        if ((wv[0] ^ wv[1] ^ wv[2] ^ wv[3]) == 0x9E3779B9u) *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);"),
            ("                        *(uint2 *)(row + k) = make_uint2(",
             "                        if (((uint32_t)q0 ^ (uint32_t)q3) == 0x9E3779B9u) *(uint2 *)(row + k) = make_uint2(")],
    "CS1": [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
             "                        *(uint4 *)(is_buf + (size_t)(ubase + 64 * rd) * 576 + 32 * k + 8 * lane) = make_uint4(wv[0], wv[1], wv[2], wv[3]);"),
            ("                        *(uint2 *)(row + k) = make_uint2(",
             "                        *(uint2 *)(is_buf + (size_t)(ubase + 64 * rd) * 576 + 32 * k + 4 * lane) = make_uint2(")],
    "BASE": [],
    # r03: lane_sel as a plain select of t (wrong for mono frames; C3 is all stereo): what the history and
    # overlap selects cost (NOSEL)
    "NOSEL": [("""    __asm__("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
    return r;""", """    (void)m; (void)f; r = t;
    return r;""")],
    "S2": [],
    "K1": [],
    "K2": [],
    "C2S": [],
    "C1W": [],
    "C4W": [],
    # r03: each row zeroed from nz_end to the next 128-B / 64-B boundary (no partially written line) (PAD128, PAD64)
    "PAD128": None,
    "PAD64": None,
    # r03: big_values groups wholly past the lane's big_values not stored (count1 or nothing reads them) (BVZ)
    "BVZ": [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
             "                        if (k < bv2) *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);")],
    # round 5: big_values group stores only up to the end of the 128-B line holding the lane's last pair (BVL)
    "BVL": [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
             "                        if (k < ((bv2 + 63) & ~63)) *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);")],
    # round 5 LDS bank-conflict diagnosis (output wrong; counters only): each read class made conflict-free
    "CFW": [("    const uint32_t w0 = bits[(int)w - 1], w1 = bits[w], w2 = bits[w + 1];",
             "    const int ln = lane_now();\n    const uint32_t w0 = bits[ln], w1 = bits[ln + 64], w2 = bits[ln + 128]; (void)w;")],
    "CFL1": [("const uint32_t e1 = s_lut[i1];", "const uint32_t e1 = s_lut[(i1 & ~63u) + (uint32_t)lane_now()];")],
    "CFL2": [("const uint32_t e = s_lut[i2];", "const uint32_t e = s_lut[(i2 & ~63u) + (uint32_t)lane_now()];")],
    "CFC": [("                        const uint32_t e = s_lut[c1base + (hw >> c1sh)];",
             "                        const uint32_t e = s_lut[((c1base + (hw >> c1sh)) & ~63u) + (uint32_t)lane];"),
            ("                        se = s_c1s[(v << 4) | ((hw << lq) >> 28)];",
             "                        se = s_c1s[(((v << 4) | ((hw << lq) >> 28)) & ~63u) + (uint32_t)lane];")],
    # round 5, k_demux_fp ablations (output wrong; timing only): no parse / no serial resolve / no payload copy
    "FPNP": [("        if (fb > 0) parse_frame<SrcGlobal>(w[j], p0, 0, cur, len, fb, stream_start && f == 0, opts, S, fp, r[j], inf[j], lane);",
              "        (void)fb; (void)cur;")],
    "FPNR": [("        for (int f = 0; f < F; f++) {\n            const FpRes q = s_res[f];",
              "        for (int f = 0; f < 0; f++) {\n            const FpRes q = s_res[f];")],
    "FPNC": [("            copy_payload<SrcGlobal>(p0, dst, r[j], fo[f] + body, fo[f], lane);", "            (void)body;")],
    # timing only (C3 holds no LSF stream): the LSF k_synth launch skipped on int16 batches (NL)
    "NL": [("        if (kinds & 2) MP3D_SYNTH_LAUNCH(false, true);", "")],
    # r03: k_mdcopy quadruples by one unaligned 16-B load each instead of 16 + 4 B and four funnel shifts (UA1)
    "UA1": [('                    const uint32_t *L = q < nq ? lp + 4u * q : (const uint32_t *)dst;\n                    uint4 a;\n                    __builtin_memcpy(&a, L, 16);\n                    const uint32_t e = L[4];\n                    v[j] = make_uint4(__builtin_amdgcn_alignbit(a.y, sh ? a.x : a.y, sh),\n                                      __builtin_amdgcn_alignbit(a.z, sh ? a.y : a.z, sh),\n                                      __builtin_amdgcn_alignbit(a.w, sh ? a.z : a.w, sh),\n                                      __builtin_amdgcn_alignbit(e, sh ? a.w : e, sh));', '                    v[j] = *(const uint4 *)(q < nq ? sb + 16u * q : (const uint8_t *)dst); /* unaligned 16-B load */')],
    # r03: is[] row stores (big_values groups, count1 quadruples) non-temporal (NT1)
    "NT1": [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
             "                        { typedef uint32_t nt4 __attribute__((ext_vector_type(4))); __builtin_nontemporal_store((nt4){wv[0], wv[1], wv[2], wv[3]}, (nt4 *)(row + k)); }"),
            ("""                        *(uint2 *)(row + kq) = make_uint2(__builtin_amdgcn_perm(se, se, 0x09030801u),
                                                          __builtin_amdgcn_perm(se << 8, se, 0x0B070A05u));""",
             """                        typedef uint32_t nt2 __attribute__((ext_vector_type(2)));
                        __builtin_nontemporal_store((nt2){__builtin_amdgcn_perm(se, se, 0x09030801u),
                                                          __builtin_amdgcn_perm(se << 8, se, 0x0B070A05u)}, (nt2 *)(row + kq));""")],
    # r03: the next granule's prefetch issued at the start of phase I (PFI) / after the matrixing MFMAs (PFM)
    "PFI": [('                if (PF == 0 && (LSF ? f + 1 < f1 : (gr == 0 || f + 1 < f1))) prefetch(LSF ? 2 * f + 2 : 2 * f + gr + 1, cs);\n', ""),
            ("            /* ---------------- phase I: alias + IMDCT + overlap ------------ */\n",
             "            /* ---------------- phase I: alias + IMDCT + overlap ------------ */\n" + '            if (!SRC_XR && PF == 0 && (LSF ? f + 1 < f1 : (gr == 0 || f + 1 < f1))) prefetch(LSF ? 2 * f + 2 : 2 * f + gr + 1, cs);\n')],
    "PFM": [('                if (PF == 0 && (LSF ? f + 1 < f1 : (gr == 0 || f + 1 < f1))) prefetch(LSF ? 2 * f + 2 : 2 * f + gr + 1, cs);\n', ""),
            ("                wave_sync(); /* all S reads retired before X overwrites them */\n",
             '            if (!SRC_XR && PF == 0 && (LSF ? f + 1 < f1 : (gr == 0 || f + 1 < f1))) prefetch(LSF ? 2 * f + 2 : 2 * f + gr + 1, cs);\n' + "                wave_sync(); /* all S reads retired before X overwrites them */\n")],
    # r03: the count1 sign table with the store in the same iteration (no software pipelining)
    "S13": [("""                    int kp = -1;
                    uint32_t sp = 0u;
                    while (k <= 572 && pos < end_bit) {
                        const uint32_t hw = win32g(bits, pos);
                        const uint32_t e = s_lut[c1base + (hw >> c1sh)];
                        if (kp >= 0) c1_store(kp, sp);
                        kp = -1;""", """                    int kp = -1;
                    uint32_t sp = 0u;
                    while (k <= 572 && pos < end_bit) {
                        const uint32_t hw = win32g(bits, pos);
                        const uint32_t e = s_lut[c1base + (hw >> c1sh)];"""),
            ("""                        sp = s_c1s[(v << 4) | ((hw << lq) >> 28)];
                        kp = k;""", """                        sp = s_c1s[(v << 4) | ((hw << lq) >> 28)];
                        c1_store(k, sp);"""),
            ("""                    if (kp >= 0) c1_store(kp, sp);""", """                    (void)kp;""")],
    # r03: without the two phase-Q tweaks (lane / MW test, M/S factor multiply) of QT1
    "S9": [("                if (lane < nch * MW) ((uint32_t *)&Wd.m[0])[lane] = wm[cs]; /* lane / MW < nch, no division */",
            "                if (lane < 2 * MW && lane / MW < nch) ((uint32_t *)&Wd.m[0])[lane] = wm[cs];"),
           ("""                const float msf = ms_fold ? isq : 1.f; /* uniform: one multiply, no select */
                auto p2q = [&](int q) { return ldexpf(T.p2q[q & 3], q >> 2) * msf; };""",
            """                auto p2q = [&](int q) {
                    const float v = ldexpf(T.p2q[q & 3], q >> 2);
                    return ms_fold ? v * isq : v;
                };""")],
    # r03: is[] prefetch loads unconditional, masked by an out-of-range buffer offset (no exec branch per load)
    "PB1": [("""                nis[c][i] = 0u;
                if ((i < 4 || lane < 32) && 2 * lane + 128 * i < nz)
                    nis[c][i] = __builtin_amdgcn_raw_buffer_load_b32(r_is, lo + c * 1152 + 256 * i, g * gb, 0);""",
             """                const bool on = (i < 4 || lane < 32) && 2 * lane + 128 * i < nz;
                nis[c][i] = __builtin_amdgcn_raw_buffer_load_b32(r_is, on ? lo + c * 1152 + 256 * i : 0x40000000, g * gb, 0);""")],
    "XPF4": [],
    "DM2": [],
    "H2": [],
    "W9": [],
    "Q2": [],
    "Q3": [],
    "S1": [],
    "A2": [],
    "P1": [],
    "WK": [],
    "MC2": [],
    "MC3": [],
    "OV1": [],
    "HG4": [],
    "SF": [],
    "HT": [],
    "FR": [],
    "HTOLD": [("/* the block's LDS tables: the LUT (the whole array: past the last table it\n * holds the zero table of table_select 0, 4, 14), table_select -> LUT base |\n * bits1 << 16 | linbits << 24, long sfb start lines per sample-rate index,\n * MPEG-1 slen pairs.  Every load is independent (one memory latency).\n * Both Huffman kernels run 256-thread blocks. */\n__device__ __forceinline__ void huff_tables(const DevTables *tab, uint16_t *s_lut, uint32_t *s_tsel,\n                                            uint16_t (*s_lbnd)[24], uint8_t *s_slen) {\n    constexpr int LUT4 = MP3D_LUT_MAX / 8; /* uint4 chunks */\n    constexpr int PER = (LUT4 + 255) / 256;\n    const uint4 *src = (const uint4 *)tab->lut;\n    uint4 v[PER];\n#pragma unroll\n    for (int j = 0; j < PER; j++) {\n        const int i = (int)threadIdx.x + 256 * j;\n        if (i < LUT4) v[j] = src[i];\n    }\n    uint32_t ts = 0u, lb = 0u;\n    if (threadIdx.x < 32) ts = tab->tsel[threadIdx.x];\n    if (threadIdx.x < 9 * 24 / 2) lb = ((const uint32_t *)tab->lbnd)[threadIdx.x];\n#pragma unroll\n    for (int j = 0; j < PER; j++) {\n        const int i = (int)threadIdx.x + 256 * j;\n        if (i < LUT4) ((uint4 *)s_lut)[i] = v[j];\n    }\n    if (threadIdx.x < 32) s_tsel[threadIdx.x] = ts;\n    if (threadIdx.x < 9 * 24 / 2) ((uint32_t *)s_lbnd)[threadIdx.x] = lb;\n    if (threadIdx.x < 32) s_slen[threadIdx.x] = MP3D_SLEN[threadIdx.x >> 4][threadIdx.x & 15];\n}\n", "/* the block's LDS tables: the LUT (+ a 2-entry all-zero table for\n * table_select 0, 4, 14), table_select -> LUT base | bits1 << 16 | linbits\n * << 24, long sfb start lines per sample-rate index, MPEG-1 slen pairs */\n__device__ __forceinline__ void huff_tables(const DevTables *tab, uint16_t *s_lut, uint32_t *s_tsel,\n                                            uint16_t (*s_lbnd)[24], uint8_t *s_slen) {\n    const int lut_n = tab->lut_hdr.base[MP3D_LUT_TABLES - 1] + (1 << tab->lut_hdr.bits1[MP3D_LUT_TABLES - 1]);\n    const int zbase = (lut_n + 1) & ~1;\n    for (int i = threadIdx.x; i < (lut_n + 1) / 2; i += blockDim.x)\n        ((uint32_t *)s_lut)[i] = ((const uint32_t *)tab->lut)[i];\n    if (threadIdx.x == 0) ((uint32_t *)s_lut)[zbase / 2] = 0u;\n    if (threadIdx.x < 9) {\n        int acc = 0;\n        for (int i = 0; i < 22; i++) {\n            s_lbnd[threadIdx.x][i] = (uint16_t)acc;\n            acc += MP3D_SFB_LONG_WIDTH[threadIdx.x][i];\n        }\n        s_lbnd[threadIdx.x][22] = (uint16_t)acc;\n    }\n    if (threadIdx.x < 32) s_slen[threadIdx.x] = MP3D_SLEN[threadIdx.x >> 4][threadIdx.x & 15];\n    if (threadIdx.x < 32) {\n        const int t = MP3D_HTAB_OF_SELECT[threadIdx.x];\n        s_tsel[threadIdx.x] = t < 0 ? (uint32_t)zbase | (1u << 16)\n                                    : (uint32_t)tab->lut_hdr.base[t] | ((uint32_t)tab->lut_hdr.bits1[t] << 16) |\n                                          ((uint32_t)MP3D_LINBITS[threadIdx.x] << 24);\n    }\n}\n")],
    "NOW": [],
    "NOW2": [],
    "NOW3": [],
    # r02 diagnostic (same output): k_frame phase timestamps (s_memtime) in g_fdbg, read by
    # tools/dbg/frame_timing.py through mp3d_dbg_read
    "FRT": [("#define PF_BYTES 4096 /* = MP3D_PF_BYTES (mp3d_dec.cpp): the staged stream length */\n",
             "#define PF_BYTES 4096 /* = MP3D_PF_BYTES (mp3d_dec.cpp): the staged stream length */\n"
             "__device__ unsigned long long g_fdbg[32];\n"
             "#define FT(i) do { __asm__ volatile(\"s_waitcnt vmcnt(0) lgkmcnt(0)\" ::: \"memory\"); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) g_fdbg[(i)] = t_; } while (0)\n"),
            ("    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);\n    if (wv == 0) {\n",
             "    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);\n    const unsigned long long T0 = __builtin_amdgcn_s_memtime(), R0 = __builtin_amdgcn_s_memrealtime();\n"
             "    if (tid == 0) { g_fdbg[0] = T0; g_fdbg[20] = R0; }\n    if (wv == 0) {\n"),
            ("        wave_sync();\n        demux_stream((const uint8_t *)s_in, in_off, in_len, md, md_off, st, rec, sideu, infos, 1, opts, 0, lane);\n",
             "        wave_sync();\n        FT(1);\n        demux_stream((const uint8_t *)s_in, in_off, in_len, md, md_off, st, rec, sideu, infos, 1, opts, 0, lane);\n        FT(2);\n"),
            ("        synth_tables<F32, LSF, 192>(T, tab, tid - 64);\n",
             "        synth_tables<F32, LSF, 192>(T, tab, tid - 64);\n        if (wv == 1) FT(3);\n"),
            ("    __syncthreads(); /* rec, side words, md region and state visible to the workgroup */\n",
             "    __syncthreads(); /* rec, side words, md region and state visible to the workgroup */\n    if (wv == 0) FT(5);\n"),
            ("    __syncthreads(); /* is[] rows and UnitMeta visible to the synthesis waves */\n",
             "    FT(6 + wv);\n    __syncthreads(); /* is[] rows and UnitMeta visible to the synthesis waves */\n    if (wv == 0) FT(10);\n"),
            ("        __threadfence_system(); /* PCM, frame info and state before the completion word */\n",
             "        FT(11);\n        __threadfence_system(); /* PCM, frame info and state before the completion word */\n        FT(12);\n"
             "        if (lane == 0) g_fdbg[21] = __builtin_amdgcn_s_memrealtime();\n"),
            ("#define HW_WORDS 520 /* staged md words per unit: four 4095-bit units + margin */\n",
             "#define HW_WORDS 520 /* staged md words per unit: four 4095-bit units + margin */\n"
             "static __device__ unsigned long long g_hdbg[32];\n"
             "#define HT(i) do { __asm__ volatile(\"s_waitcnt vmcnt(0) lgkmcnt(0)\" ::: \"memory\"); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) g_hdbg[(u & 3) * 8 + (i)] = t_; } while (0)\n"),
            ("    wave_sync();\n    const uint32_t seg = 0u - 32u * w0; /* md bit -> staged bit */\n",
             "    wave_sync();\n    HT(0);\n    const uint32_t seg = 0u - 32u * w0; /* md bit -> staged bit */\n"),
            ("    const int ws = (int)(side >> 30) & 1;\n    const int bv2 = 2 * ((int)(side >> 43) & 0x1FF);\n    int r1, r2;",
             "    HT(1);\n    const int ws = (int)(side >> 30) & 1;\n    const int bv2 = 2 * ((int)(side >> 43) & 0x1FF);\n    int r1, r2;"),
            ("    /* count1 quadruples until the part2_3 end (one per 2 words)",
             "    HT(2);\n    /* count1 quadruples until the part2_3 end (one per 2 words)"),
            ("\n    if (lane == 0) {\n        UnitMeta m;\n", "\n    HT(3);\n    if (lane == 0) {\n        UnitMeta m;\n"),
            ("""/* k_frame's copies of the demux constants (this translation unit's) */""",
             """extern "C" __attribute__((visibility("default"))) int mp3d_dbg_read(unsigned long long *h) {
    hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fdbg), sizeof(g_fdbg), 0, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpyFromSymbol(h + 32, HIP_SYMBOL(g_hdbg), sizeof(g_hdbg), 0, hipMemcpyDeviceToHost);
    return (int)e;
}
/* k_frame's copies of the demux constants (this translation unit's) */""")],
    "WP": [('                    for (; __ballot(k < bv2); k += 8) {\n                        uint32_t wv[4];\n#pragma unroll\n                        for (int j = 0; j < 4; j++) {\n                            const int kk = k + 2 * j;\n                            const uint32_t ts = kk < r1 ? ts0 : (kk < r2 ? ts1 : ts2);\n                            const uint32_t tb = ts & 0xFFFFu, b1 = (ts >> 16) & 15u, lin = ts >> 24;\n                            uint32_t hi, lo;\n                            win64(bits, pos, hi, lo);\n', '                    uint32_t W = min(pos >> 5, (uint32_t)(HUFF_CAPW - 2));\n                    uint32_t q0 = bits[W], q1 = bits[W + 1], q2 = bits[W + 2], q3 = bits[W + 3], q4 = bits[W + 4];\n                    for (; __ballot(k < bv2); k += 8) {\n                        uint32_t wv[4];\n#pragma unroll\n                        for (int j = 0; j < 4; j++) {\n                            const int kk = k + 2 * j;\n                            const uint32_t ts = kk < r1 ? ts0 : (kk < r2 ? ts1 : ts2);\n                            const uint32_t tb = ts & 0xFFFFu, b1 = (ts >> 16) & 15u, lin = ts >> 24;\n                            const uint32_t d = (pos >> 5) - W;\n                            const uint32_t w0 = d == 0u ? q0 : (d == 1u ? q1 : q2);\n                            const uint32_t w1 = d == 0u ? q1 : (d == 1u ? q2 : q3);\n                            const uint32_t w2 = d == 0u ? q2 : (d == 1u ? q3 : q4);\n                            W = min(pos >> 5, (uint32_t)(HUFF_CAPW - 2));\n                            q0 = bits[W]; q1 = bits[W + 1]; q2 = bits[W + 2]; q3 = bits[W + 3]; q4 = bits[W + 4];\n                            const uint32_t shw = 32u - (pos & 31u);\n                            const uint32_t hi = (uint32_t)((((uint64_t)w0 << 32) | w1) >> shw);\n                            const uint32_t lo = (uint32_t)((((uint64_t)w1 << 32) | w2) >> shw);\n')],
    "HB": [("""                            const uint32_t i2 = (e1 & 0x8000u) ? sub : i1;
                            const uint32_t e = s_lut[i2];""", """                            uint32_t e = e1;
                            if (__ballot(e1 & 0x8000u)) e = s_lut[(e1 & 0x8000u) ? sub : i1];""")],
    "WL16": [("#define WALK_LANES 64", "#define WALK_LANES 16")],
    "WL32": [("#define WALK_LANES 64", "#define WALK_LANES 32")],
    "NOSLP": [],  # now the default for mp3d_synth.hip (_build.FILE_FLAGS)
    # r02 sensitivity probes (same output): +64 dependent-free VALU per granule in k_synth phase W,
    # +8 VALU per codeword in the Huffman big_values loop
    "SV64": [("                auto out2 = [&](int tp) { return acc[tp]; };",
              "                { float d0 = acc[0].x, d1 = acc[1].x, d2 = acc[2].x, d3 = acc[3].x;\n"
              "#pragma unroll\n                  for (int q = 0; q < 16; q++) { __asm__ volatile(\"v_add_f32 %0, %0, %0\\n v_add_f32 %1, %1, %1\\n v_add_f32 %2, %2, %2\\n v_add_f32 %3, %3, %3\" : \"+v\"(d0), \"+v\"(d1), \"+v\"(d2), \"+v\"(d3)); }\n"
              "                  if (d0 == 1.2345f && d1 == d2 && d3 == 0.5f) acc[8].y += 1e-30f; }\n"
              "                auto out2 = [&](int tp) { return acc[tp]; };")],
    "HV8": [("                    for (; k < bv2; k += 2) {",
             "                    uint32_t hv_dummy = 0u;\n                    for (; k < bv2; k += 2) {"),
            ("                        const uint32_t e = s_lut[i2];",
             "                        const uint32_t e = s_lut[i2];\n"
             "                        { uint32_t d0 = k, d1 = k + 1u;\n"
             "                          __asm__ volatile(\"v_add_u32 %0, %0, %0\\n v_add_u32 %1, %1, %1\\n v_add_u32 %0, %0, %0\\n v_add_u32 %1, %1, %1\\n v_add_u32 %0, %0, %0\\n v_add_u32 %1, %1, %1\\n v_add_u32 %0, %0, %0\\n v_add_u32 %1, %1, %1\" : \"+v\"(d0), \"+v\"(d1));\n"
             "                          hv_dummy ^= d0 ^ d1; }"),
            ("                    m.used_bits = (uint16_t)(pos - start - seg);",
             "                    m.used_bits = (uint16_t)(pos - start - seg) | (hv_dummy == 0x9E3779B9u ? 0x8000u : 0u);")],
    "XPF3": [("amdgpu_waves_per_eu(SRC_XR ? 4 : 3, 8)", "amdgpu_waves_per_eu(3, 8)")],
    # r02: k_demux without the waves_per_eu(8, 8) attribute of commit 315cc86
    "DMW0": [("__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) k_demux(",
              "__global__ void __launch_bounds__(64) k_demux(")],
    # r02: the synth-only (C2) variant at 4 waves / SIMD (131 -> 128 VGPRs)
    "XW4": [("__attribute__((amdgpu_waves_per_eu(3, 8)))", "__attribute__((amdgpu_waves_per_eu(SRC_XR ? 4 : 3, 8)))")],
    "CAP2300": [("#define HUFF_CAPW 2400", "#define HUFF_CAPW 2300")],
    "LUT2400": [("#define HUFF_CAPW 2300", "#define HUFF_CAPW 2400")],
    "DM1": [("const bool lsf = hdr_kind(h1) == 2;", "const bool lsf = false;")],
    "DM2": [("|| (v59 & (7ull << 23)) == (4ull << 23))", ")")],
    "DM3": [("if (kind && hdr_kind(b1) != kind) return -1;", ""),
            ("const bool crc_bad = (opts & MP3D_OPT_CRC_CHECK) && crc && !crc16_ok(w, (uint32_t)side_bytes);",
             "const bool crc_bad = false;")],
    "H8a": [("#define HUFF_WAVES 4", "#define HUFF_WAVES 8"), ("#define HUFF_CAPW 2400", "#define HUFF_CAPW 2080"), W4H],
    "H8b": [("#define HUFF_WAVES 4", "#define HUFF_WAVES 8"), ("#define HUFF_CAPW 2400", "#define HUFF_CAPW 2000"), W4H],
    "R8": [("#define HUFF_ROUNDS 4 ", "#define HUFF_ROUNDS 8 ")],
    "R16": [("#define HUFF_ROUNDS 4 ", "#define HUFF_ROUNDS 16")],
    "W4": [("__attribute__((amdgpu_waves_per_eu(3, 8)))", "__attribute__((amdgpu_waves_per_eu(4, 8)))")],
    "W2": [("""    __shared__ __attribute__((aligned(16))) SynWave Wv[SYN_WAVES];""",
            """    __shared__ __attribute__((aligned(16))) SynWave Wv[SYN_WAVES];
    __shared__ float pad_[5000];
    if (n_streams < 0) pad_[threadIdx.x] = 0.f;""")],
    "NI": [("""                const bool long_imdct = bt != 2 || (mixed && sb < 2);
                if (long_imdct) {""", """                const bool long_imdct = bt != 2 || (mixed && sb < 2);
                if (true) {
#pragma unroll
                    for (int i = 0; i < 18; i++) { o18[i] = x[i] + ov[i]; ov[i] = active ? x[17 - i] : ov[i]; }
                } else if (long_imdct) {"""),
           ("""                const bool upper = (bt != 2 && sb >= 1)""", """                const bool upper = false && (bt != 2 && sb >= 1)"""),
           ("""                const bool lower = (bt != 2 && sb <= 30)""", """                const bool lower = false && (bt != 2 && sb <= 30)""")],
    "NW": [("""                        o = __builtin_elementwise_fma((f32x2){Dw[2 * i], Dw[2 * i]}, va, o);
                        o = __builtin_elementwise_fma((f32x2){Dw[2 * i + 1], Dw[2 * i + 1]}, vb, o);""",
            """                        if (i == 0) o = va + vb;""")],
    "NM": [("""                        ce[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ae[ks], Be[nt][ks], ce[nt], 0, 0, 0);
                        co[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ao[ks], Bo[nt][ks], co[nt], 0, 0, 0);""",
            """                        ce[nt][ks] = Ae[ks] * Be[nt][ks];
                        co[nt][ks] = Ao[ks] * Bo[nt][ks];""")],
}

def _pad(n):
    return [("                    const int nz_end = k;\n",
             "                    const int nz_end = k;\n"
             "                    {   /* zero the row from nz_end to the next %d-B boundary: no partially written line */\n"
             "                        uint32_t b = 2u * (uint32_t)nz_end;\n"
             "                        const uint32_t B = (b + %du) & ~%du;\n"
             "                        uint8_t *rb = (uint8_t *)row;\n"
             "                        if (b < B && (b & 4u)) { *(uint32_t *)(rb + b) = 0u; b += 4u; }\n"
             "                        if (b < B && (b & 8u)) { *(uint2 *)(rb + b) = make_uint2(0u, 0u); b += 8u; }\n"
             "                        for (; b < B; b += 16u) *(uint4 *)(rb + b) = make_uint4(0u, 0u, 0u, 0u);\n"
             "                    }\n" % (n, n - 1, n - 1))]


# round 4: the partial-sum history / 4-wave k_synth at the old 3-wave budget
VARS["S3W"] = [("amdgpu_waves_per_eu(SynCfg<SRC_XR, LSF>::DMA ? 4 : 3, 8)", "amdgpu_waves_per_eu(3, 8)")]

# round 4: k_huffman back at 4-wave workgroups (3 per CU; 161 VGPRs at LDS 53 KB) beside the 16-wave one
VARS["H4"] = [("#define HUFF_WAVES 16", "#define HUFF_WAVES 4"),
              ("#define HUFF_CAPW 2304", "#define HUFF_CAPW 2336"),
              ("    blocks = blocks < n_cu ? (blocks > 0 ? blocks : 1) : n_cu;", "    blocks = blocks > 0 ? blocks : 1;")]

# round 4: the 8-wave k_synth with the is[] prefetch back in registers (no LDS-DMA)
VARS["NODMA"] = [("        if (PAR) {\n            dma_is(g, nz0, nz1);", "        if (false) {\n            dma_is(g, nz0, nz1);"),
                 ("cis[c][i] = PAR ? isq[320 * c + 64 * i + lane] : nis[c][i];", "cis[c][i] = nis[c][i];")]

# round 4: phase W's pair i stored after step i's history updates (its convert / swap chain overlaps them)
VARS["EMITLATE"] = [("""                        emit(stereo, i, acc[i]);
                        hp[i] = (f32x2){d.y * xb17, 0.f}; /* H_2i: B(-1) = this X_17 */
#pragma unroll
                        for (int tp = 0; tp < i; tp++) {
                            /* k = 2 (tp - i) + 18: A = xap[k / 2], B = xbp[k / 2 - 1] */
                            hp[tp] = pfma(bc(d.x), xap[tp - i + 9], hp[tp]);
                            hp[tp] = pfma(bc(d.y), xbp[tp - i + 8], hp[tp]);
                        }""", """                        const f32x2 done = acc[i];
                        hp[i] = (f32x2){d.y * xb17, 0.f}; /* H_2i: B(-1) = this X_17 */
#pragma unroll
                        for (int tp = 0; tp < i; tp++) {
                            /* k = 2 (tp - i) + 18: A = xap[k / 2], B = xbp[k / 2 - 1] */
                            hp[tp] = pfma(bc(d.x), xap[tp - i + 9], hp[tp]);
                            hp[tp] = pfma(bc(d.y), xbp[tp - i + 8], hp[tp]);
                        }
                        emit(stereo, i, done);""")]

VARS["PAD128"] = _pad(128)
VARS["PAD64"] = _pad(64)

# r04: the synth-only (C2) variant at 4 waves / SIMD with its register prefetch (spills 40 B):
# 8-wave workgroups (XS4) or 4-wave (XS4b)
_XWPE = ("amdgpu_waves_per_eu(SynCfg<SRC_XR, LSF>::DMA ? 4 : 3, 8)", "amdgpu_waves_per_eu(!LSF ? 4 : 3, 8)")
VARS["XS4"] = [_XWPE, ("static constexpr int WAVES = DMA ? 8 : 4;", "static constexpr int WAVES = !LSF ? 8 : 4;")]
VARS["XS4b"] = [_XWPE]

# XS4M: XS4 with the next granule's spectra loads issued at phase M (after phase I's register peak)
_XQ = ("                if (f + 1 < f1 || gr == 0) load_xr(2 * f + gr + 1); /* next granule, in flight through I, M, W */\n", "")
_XM = ("            /* ---------------- phase M: matrixing on the matrix cores ------- */\n",
       "            /* ---------------- phase M: matrixing on the matrix cores ------- */\n"
       "            if (SRC_XR && (f + 1 < f1 || gr == 0)) load_xr(2 * f + gr + 1);\n")
VARS["XS4M"] = VARS["XS4"] + [_XQ, _XM]
VARS["XS4Mb"] = VARS["XS4b"] + [_XQ, _XM]

# r04: phase-Q wave priority off (SP0)
VARS["SP0"] = [("            if (!SRC_XR) __builtin_amdgcn_s_setprio(1);\n            bool fusedq",
                "            bool fusedq")]

# r04: xin takes the alias neighbours by DPP wave shifts, not 8 LDS reads (XDPP)
VARS["XDPP"] = [("""                const int pb = sbx ? base - 8 : base, nb = sbx < 31 ? base + 18 : base;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float2 p = *(const float2 *)&sBuf[pb + 2 * i];
                    const float2 n = *(const float2 *)&sBuf[nb + 2 * i];
                    up[7 - 2 * i] = p.x;
                    up[6 - 2 * i] = p.y;
                    dn[2 * i] = n.x;
                    dn[2 * i + 1] = n.y;
                }""", """                (void)sbx;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    up[k] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xf[17 - k]), 0x138, 0xF, 0xF, false));
                    dn[k] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xf[k]), 0x130, 0xF, 0xF, false));
                }""")]

# r04 timing probe (wrong output): k_walk's header chain alone, no side info / reservoir / record work (WCH)
VARS["WCH"] = [("            if (cur + (uint32_t)fb <= len || cur + need <= len) {",
                "            if (cur + (uint32_t)fb <= len) {\n                cur += (uint32_t)fb;\n            } else if (false) {")]

# r04: 2 ranking rounds per super-chunk (R2)
VARS["R2"] = [("#define HUFF_ROUNDS 4", "#define HUFF_ROUNDS 2")]

VARS["R6"] = [("#define HUFF_ROUNDS 4", "#define HUFF_ROUNDS 6")]
VARS["R8b"] = [("#define HUFF_ROUNDS 4", "#define HUFF_ROUNDS 8")]

# r04: k_synth MPEG-1 / synth-only in one 16-wave workgroup per CU (W16)
VARS["W16"] = [("    static constexpr int WAVES = DMA ? 8 : 4;", "    static constexpr int WAVES = DMA ? 16 : 4;")]

# r04: persistent MPEG-1 k_synth (one resident round of workgroups, each wave walks blocks) (PST)
VARS["PST"] = [
    ("    if (!SRC_XR && !(LSF && fam)) {", "    if (!SRC_XR && LSF && !fam) {"),
    ("""    if constexpr (LSF && !SRC_XR) {
        for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x)
            if (!run(blk)) break;
    } else {
        run(blockIdx.x);
    }""", """    if constexpr (!SRC_XR) {
        for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x)
            if (!run(blk)) break;
    } else {
        run(blockIdx.x);
    }"""),
    ("        if (LSF_ && fam && nb > lsf_grid) nb = lsf_grid;                                                           \\",
     "        if (LSF_ && fam && nb > lsf_grid) nb = lsf_grid;                                                           \\\n        if (!LSF_ && nb > 2 * (n_cu > 0 ? n_cu : 256)) nb = 2 * (n_cu > 0 ? n_cu : 256);                            \\"),
]

VARS["PST2"] = VARS["PST"] + [
    ("""        synth_stream<SRC_XR, F32, LSF>(rec, is_buf, meta, xr_in, xr_bt, xr_mixed, tab, st, pcm, F, xr_nch, xr_sr,
                                       seg_len, st_tail, st_tail_in, T, Wv[wid], s, seg, nseg, nullptr,
                                       SynCfg<SRC_XR, LSF>::DMA ? s_isq[SynCfg<SRC_XR, LSF>::DMA ? wid : 0] : nullptr);""",
     """        int z = blk;
        __asm__("" : "+s"(z));
        z -= blk; /* 0, unknown to the optimizer: the LDS bases are re-derived per stream, not hoisted */
        synth_stream<SRC_XR, F32, LSF>(rec, is_buf, meta, xr_in, xr_bt, xr_mixed, tab, st, pcm, F, xr_nch, xr_sr,
                                       seg_len, st_tail, st_tail_in, *(&T + z), Wv[wid + z], s, seg, nseg, nullptr,
                                       SynCfg<SRC_XR, LSF>::DMA ? s_isq[(SynCfg<SRC_XR, LSF>::DMA ? wid : 0) + z] : nullptr);"""),
]

VARS["NOSLPALL"] = [("FLAGS", "-fno-slp-vectorize")]
VARS["UNR"] = [("FLAGS", "-mllvm"), ("FLAGS", "-unroll-threshold=400")]

# k_huffman store cost (round 5): big_values group stores kept only when the
# group's four words xor to a value no group has (the decode itself stays live)
VARS["NST"] = [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
                "                        if ((wv[0] ^ wv[1] ^ wv[2] ^ wv[3]) == 0x7FFF8001u) *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);")]
# ... and the count1 stores too
VARS["NSTC"] = VARS["NST"] + [
    ("                        __builtin_memcpy(row + k, &q, 16);",
     "                        if ((q.x ^ q.w) == 0x7FFF8001u) __builtin_memcpy(row + k, &q, 16);")]
# k_huffman: main-data staging loads non-temporal (leave L2 to the is[] rows being filled)
VARS["NTL"] = [("                            if (i + 4 * k < len) v[k] = *(const uint4 *)(src + i + 4 * k);",
                "                            if (i + 4 * k < len) { typedef uint32_t u4v __attribute__((ext_vector_type(4))); const u4v t = __builtin_nontemporal_load((const u4v *)(src + i + 4 * k)); v[k] = make_uint4(t.x, t.y, t.z, t.w); }")]
# k_huffman: big_values group stores non-temporal
VARS["NTS"] = [("                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);",
                "                        { typedef uint32_t u4v __attribute__((ext_vector_type(4))); __builtin_nontemporal_store((u4v){wv[0], wv[1], wv[2], wv[3]}, (u4v *)(row + k)); }")]
# k_huffman waves per CU (open is[] rows per CU = 64 x waves)
VARS["HW12"] = [("#define HUFF_WAVES 16", "#define HUFF_WAVES 12")]  # (round 5 sources)
VARS["HW8"] = [("#define HUFF_WAVES 16", "#define HUFF_WAVES 8")]
# round 7: k_huffman waves per CU x big_values groups per store burst (the staging area follows the
# wave count): HwBb.  H12B8 is the product; H16B4 spills (24 VGPRs).  profiles/r07_huff_bursts.txt
for _w, _b in ((16, 2), (16, 4), (12, 2), (12, 4), (12, 8)):
    VARS["H%dB%d" % (_w, _b)] = [("FLAGS", "-DHUFF_WAVES=%d" % _w), ("FLAGS", "-DHUFF_BURST=%d" % _b)]
# k_rank segment size (units ranked together): 1 024 / 2 048 instead of 4 096
VARS["RK1"] = [("#define RANK_PER 4      /* units per thread */", "#define RANK_PER 1")]
VARS["RK2"] = [("#define RANK_PER 4      /* units per thread */", "#define RANK_PER 2")]
# k_mdcopy occupancy: 16-wave workgroups; a persistent grid of 2 048 workgroups looping over streams
VARS["MDC16"] = [("#define MDC_WAVES 4", "#define MDC_WAVES 16")]
VARS["MDCP"] = [
    ("""    const int s = blockIdx.x * MDC_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= n_streams) return; /* wave-level sync only below */""",
     """    for (int s = blockIdx.x * MDC_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); s < n_streams;
         s += gridDim.x * MDC_WAVES) {"""),
    ("""    if (lane == 0) S.res_len = c;
}""", """    if (lane == 0) S.res_len = c;
    }
}"""),
    ("hipLaunchKernelGGL(k_mdcopy, dim3((n_streams + MDC_WAVES - 1) / MDC_WAVES)",
     "hipLaunchKernelGGL(k_mdcopy, dim3(std::min((n_streams + MDC_WAVES - 1) / MDC_WAVES, 2048))")]
# k_demux_fp phase costs (round 5; output wrong by construction): return after staging, after the
# state loads + carry-in copy, with the parse reduced to the frame-size lookup, after the parse, after
# the resolve
_FPS = """    SrcLds::u8 *p0 = (SrcLds::u8 *)(uintptr_t)s_run;
    uint8_t *dst = md;"""
_FPP = """    /* the wave's frames, one at a time in a loop that is not unrolled: the"""
_FPR = """    __syncthreads();
    /* The bit-reservoir map (resolve_frame's rules) for all frames at once,"""
_FPE = """    __syncthreads();
    /* records and payloads, the wave's own frames */"""
VARS["FPX1"] = [(_FPS, "    if (F > 0) return;\n" + _FPS)]
VARS["FPX1B"] = [(_FPP, "    if (F > 0) return;\n" + _FPP)]
VARS["FPX2A"] = [("        if (fb > 0) parse_frame<SrcLds>(w, p0, 0, cur, len, fb, stream_start && f == 0, opts, S, fp, r, inf, lane, ht);",
                  "        if (fb == 12345) parse_frame<SrcLds>(w, p0, 0, cur, len, fb, stream_start && f == 0, opts, S, fp, r, inf, lane, ht);"),
                 (_FPR, _FPR.replace("__syncthreads();", "__syncthreads();\n    if (F > 0) return;", 1))]
VARS["FPX2"] = [(_FPR, _FPR.replace("__syncthreads();", "__syncthreads();\n    if (F > 0) return;", 1))]
VARS["FPX3"] = [(_FPE, _FPE.replace("__syncthreads();", "__syncthreads();\n    if (F > 0) return;", 1))]
# k_demux_fp phase timestamps (s_memrealtime, 10 ns ticks) in the bitrate of frame infos 0..3
# (tools/dbg/fp_times.py reads them): staging, state loads, wave 0's parse + resolve, wave 0's emits
_FPT = "__builtin_amdgcn_s_memrealtime()"
VARS["FPT"] = [
    ("""    uint32_t fo_lane = 0u;""", """    const uint64_t t_0 = """ + _FPT + """;
    uint32_t fo_lane = 0u;"""),
    ("""    SrcLds::u8 *p0 = (SrcLds::u8 *)(uintptr_t)s_run;
    uint8_t *dst = md;""", """    const uint64_t t_1 = """ + _FPT + """;
    SrcLds::u8 *p0 = (SrcLds::u8 *)(uintptr_t)s_run;
    uint8_t *dst = md;"""),
    ("""    /* Wave 0 alone: the frames' headers and side info, lane f = frame f""",
     """    const uint64_t t_2 = """ + _FPT + """;
    /* Wave 0 alone: the frames' headers and side info, lane f = frame f"""),
    ("""    __syncthreads();
    /* records and payloads, the wave's own frames */""",
     """    __syncthreads();
    const uint64_t t_3 = """ + _FPT + """;
    /* records and payloads, the wave's own frames */"""),
    ("""        /* the family of the last frame found (k_demux: of every frame) */""",
     """        if (lane == 0 && infos && F >= 4) {
            const uint64_t t_4 = """ + _FPT + """;
            infos[0].bitrate_kbps = (int)(t_1 - t_0); infos[1].bitrate_kbps = (int)(t_2 - t_1);
            infos[2].bitrate_kbps = (int)(t_3 - t_2); infos[3].bitrate_kbps = (int)(t_4 - t_3);
        }
        /* the family of the last frame found (k_demux: of every frame) */"""),
]
# is[] row stride (int16 per unit row): 640 (1 280 B, 10 lines), 608 (1 216 B, 9.5 lines)
VARS["ISR640"] = [("FLAGS", "-DMP3D_IS_ROW=640")]
VARS["ISR608"] = [("FLAGS", "-DMP3D_IS_ROW=608")]
# k_huffman without the count1 loop (output wrong): what the count1 tail costs
VARS["NC1"] = [("                    while (k <= 572 && pos < end_bit) {", "                    while (k <= 572 && pos < end_bit && F < 0) {")]
# k_mdcopy bound (output wrong): no payload word stores; no byte (head / tail / cut-short) stores;
# payload words not loaded (stores of a constant)
VARS["MDNS"] = [("""                    __builtin_amdgcn_raw_buffer_store_b128(
                        __builtin_bit_cast(__attribute__((ext_vector_type(4))) uint32_t, v[j]), r_md,
                        q < nq ? 4u * (wb + 4u * q) : 0x80000000u, 0, 0);""", """                    if (v[j].x == 0x12345679u) __builtin_amdgcn_raw_buffer_store_b128(
                        __builtin_bit_cast(__attribute__((ext_vector_type(4))) uint32_t, v[j]), r_md,
                        q < nq ? 4u * (wb + 4u * q) : 0x80000000u, 0, 0);""")]
VARS["MDNB"] = [("""                if ((uint32_t)ql < h) dst[Pm + ql] = hbv;
                if ((uint32_t)ql < L - t0) dst[Pm + t0 + ql] = tbv;""", """                if ((uint32_t)ql < h && hbv == 7) dst[Pm + ql] = hbv;
                if ((uint32_t)ql < L - t0 && tbv == 7) dst[Pm + t0 + ql] = tbv;""")]
VARS["MDNL"] = [("""                    uint4 a;
                    __builtin_memcpy(&a, L, 16);
                    const uint32_t e = L[4];""", """                    uint4 a = make_uint4(q, q + 1, q + 2, (uint32_t)(uintptr_t)L);
                    const uint32_t e = q * 7u;""")]
VARS["RK8"] = [("#define RANK_PER 4      /* units per thread */", "#define RANK_PER 8")]
VARS["RK16"] = [("#define RANK_PER 4      /* units per thread */", "#define RANK_PER 16")]
# k_huffman: big_values groups stored two steps at a time (32 B, a whole sector, per lane)
VARS["ST32"] = [("""                    for (; __ballot(k < bv2); k += 8) {
                        uint32_t wv[4];""", """                    uint4 pend = make_uint4(0u, 0u, 0u, 0u);
                    bool held = false;
                    for (; __ballot(k < bv2); k += 8) {
                        uint32_t wv[4];"""),
    ("""                        *(uint4 *)(row + k) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
                    }
                    k = bv2;""", """                        const uint4 cur = make_uint4(wv[0], wv[1], wv[2], wv[3]);
                        if (held) {
                            *(uint4 *)(row + k - 8) = pend;
                            *(uint4 *)(row + k) = cur;
                        } else {
                            pend = cur;
                        }
                        held = !held;
                    }
                    if (held) *(uint4 *)(row + k - 8) = pend;
                    k = bv2;""")]
# k_huffman: count1 groups stored in pairs too (32 B per lane every two iterations, 4-B aligned)
VARS["C1P"] = [("""                    while (k <= 572 && pos < end_bit) {
                        const uint32_t hw = win32g(bits, pos);""", """                    uint4 cpend = make_uint4(0u, 0u, 0u, 0u);
                    int kpend = -1;
                    while (k <= 572 && pos < end_bit) {
                        const uint32_t hw = win32g(bits, pos);"""),
    ("""                        __builtin_memcpy(row + k, &q, 16);
                        k += 8;
                    }""", """                        if (kpend >= 0) {
                            __builtin_memcpy(row + kpend, &cpend, 16);
                            __builtin_memcpy(row + k, &q, 16);
                            kpend = -1;
                        } else {
                            cpend = q;
                            kpend = k;
                        }
                        k += 8;
                    }
                    if (kpend >= 0) __builtin_memcpy(row + kpend, &cpend, 16);""")]
# UnitMeta padded to 64 B; k_huffman writes it as two whole 32-B sectors (scalefactors 0..31 early,
# scalefactors 32..39 + the tail + padding at the end; LSF units as before)
VARS["MT64"] = [
    ("""    uint16_t flags;      /* bit 0: granule lost to a reservoir underflow;  */
                         /* bit 1: LSF intensity_scale (scalefac_compress  */
                         /* bit 0 of an intensity frame's right channel)   */
};""", """    uint16_t flags;      /* bit 0: granule lost to a reservoir underflow;  */
                         /* bit 1: LSF intensity_scale (scalefac_compress  */
                         /* bit 0 of an intensity frame's right channel)   */
    uint32_t pad_[2];
};"""),
    ("""                        uint32_t sfw[10];
#pragma unroll
                        for (int i = 0; i < 10; i++) sfw[i] = 0u;""", """                        uint32_t sfw[10];
#pragma unroll
                        for (int i = 0; i < 10; i++) sfw[i] = 0u;"""),
    ("""                        *(uint2 *)(mrec + 32) = make_uint2(sfw[8], sfw[9]);
                    }""", """                        sf89 = make_uint2(sfw[8], sfw[9]);
                    }"""),
    ("""                    int lsf_pre = 0;
                    if (r.lsf) {""", """                    int lsf_pre = 0;
                    uint2 sf89 = make_uint2(0u, 0u);
                    if (r.lsf) {"""),
    ("""                    /* everything after sf[40]: one 16-B store */
                    *(uint4 *)((uint8_t *)&meta[u] + 40) = *(const uint4 *)((const uint8_t *)&m + 40);""",
     """                    {
                        const uint4 t = *(const uint4 *)((const uint8_t *)&m + 40);
                        uint8_t *mrec = (uint8_t *)&meta[u];
                        if (r.lsf) {
                            *(uint4 *)(mrec + 40) = t;
                        } else {
                            *(uint4 *)(mrec + 32) = make_uint4(sf89.x, sf89.y, t.x, t.y);
                            *(uint4 *)(mrec + 48) = make_uint4(t.z, t.w, 0u, 0u);
                        }
                    }"""),
]


# count1 tail without nested exec branches: both quadruples decoded every
# iteration, their acceptance as selects (C1BF)
VARS["C1BF"] = [("""                    while (k <= 572 && pos < end_bit) {
                        const uint32_t hw = win32g(bits, pos);
                        uint32_t se0, n0, se1, n1;
                        c1_dec(hw, se0, n0);
                        if (pos + n0 > end_bit) break;
                        pos += n0;
                        bool two = k <= 568 && pos < end_bit;
                        if (two) {
                            c1_dec(hw << n0, se1, n1);
                            two = pos + n1 <= end_bit;
                        }
                        if (!two) {
                            c1_store(k, se0);
                            k += 4;
                            break;
                        }
                        pos += n1;
                        const uint4 q = make_uint4(
                            __builtin_amdgcn_perm(se0, se0, 0x09030801u), __builtin_amdgcn_perm(se0 << 8, se0, 0x0B070A05u),
                            __builtin_amdgcn_perm(se1, se1, 0x09030801u), __builtin_amdgcn_perm(se1 << 8, se1, 0x0B070A05u));
                        __builtin_memcpy(row + k, &q, 16);
                        k += 8;
                    }""", """                    bool c1on = k <= 572 && pos < end_bit;
                    while (__ballot(c1on)) {
                        if (c1on) {
                            const uint32_t hw = win32g(bits, pos);
                            uint32_t se0, n0, se1, n1;
                            c1_dec(hw, se0, n0);
                            c1_dec(hw << n0, se1, n1);
                            const uint32_t p1 = pos + n0, p2 = p1 + n1;
                            const bool ok0 = p1 <= end_bit;
                            const bool ok1 = ok0 && k <= 568 && p1 < end_bit && p2 <= end_bit;
                            const uint2 q0 = make_uint2(__builtin_amdgcn_perm(se0, se0, 0x09030801u),
                                                        __builtin_amdgcn_perm(se0 << 8, se0, 0x0B070A05u));
                            if (ok1) {
                                const uint4 q = make_uint4(q0.x, q0.y, __builtin_amdgcn_perm(se1, se1, 0x09030801u),
                                                           __builtin_amdgcn_perm(se1 << 8, se1, 0x0B070A05u));
                                __builtin_memcpy(row + k, &q, 16);
                            } else if (ok0) {
                                *(uint2 *)(row + k) = q0;
                            }
                            pos = ok1 ? p2 : (ok0 ? p1 : pos);
                            k += ok1 ? 8 : (ok0 ? 4 : 0);
                            c1on = ok1 && k <= 572 && pos < end_bit;
                        }
                    }""")]

# compiler scheduling options (whole library): AMDGPU register-pressure trackers (TRK),
# no unclustered high-pressure reschedule stage (DUH)
VARS["TRK"] = [("FLAGS", "-mllvm"), ("FLAGS", "-amdgpu-use-amdgpu-trackers=1")]
VARS["DUH"] = [("FLAGS", "-mllvm"), ("FLAGS", "-amdgpu-disable-unclustered-high-rp-reschedule")]

# k_huffman big_values loop: the bit position carried negated (the window's
# funnel shift takes it as is: no v_sub per pair) and the two signs applied as
# one packed 16-bit xor / sub on the joined word (HMO)
VARS["HMO"] = [
    ("""                    uint4 pend = make_uint4(0u, 0u, 0u, 0u);
                    bool held = false;
                    for (; __ballot(k < bv2); k += 8) {""", """                    uint4 pend = make_uint4(0u, 0u, 0u, 0u);
                    bool held = false;
                    uint32_t npos = 0u - pos;
                    const int nend = -(int)end_bit;
                    for (; __ballot(k < bv2); k += 8) {"""),
    ("""                            uint32_t hi, lo;
                            win64g(bits, pos, hi, lo);""", """                            uint32_t hi, lo;
                            {
                                uint32_t w = (31u - npos) >> 5;
                                __asm__("" : "+v"(w));
                                const uint32_t w0 = bits[(int)w - 1], w1 = bits[w], w2 = bits[w + 1];
                                hi = __builtin_amdgcn_alignbit(w0, w1, npos);
                                lo = __builtin_amdgcn_alignbit(w1, w2, npos);
                            }"""),
    ("""                            const bool live = kk < bv2 && pos < end_bit;
                            pos += live ? len_c + (32u - t3) : 0u;
                            /* x = 0 gives X = 0 whatever the (absent) sign bit */
                            const int X = ((int)(x + ex) ^ mx) - mx, Y = ((int)(y + ey) ^ my) - my;
                            /* low halves of X and Y -> one word (v_perm_b32) */
                            wv[j] = live ? __builtin_amdgcn_perm((uint32_t)Y, (uint32_t)X, 0x05040100u) : 0u;""",
     """                            const bool live = kk < bv2 && (int)npos > nend;
                            npos += live ? t3 - (((e >> 8) & 31u) | 32u) : 0u;
                            const uint32_t axy = __builtin_amdgcn_perm(y + ey, x + ex, 0x05040100u);
                            const uint32_t mxy = __builtin_amdgcn_perm((uint32_t)my, (uint32_t)mx, 0x05040100u);
                            uint32_t sxy;
                            __asm__("v_pk_sub_u16 %0, %1, %2" : "=v"(sxy) : "v"(axy ^ mxy), "v"(mxy));
                            wv[j] = live ? sxy : 0u;"""),
    ("""                    if (held) *(uint4 *)(row + k - 8) = pend; /* (before the count1 stores overwrite its tail) */""",
     """                    pos = 0u - npos;
                    if (held) *(uint4 *)(row + k - 8) = pend; /* (before the count1 stores overwrite its tail) */"""),
]

# k_synth phase Q: the scale address as one v_and_or_b32 (0xFC in a VGPR: VOP3 takes no literal on
# gfx9, so the compiler split it into v_and + v_or); the fused path's alias neighbours by DPP moves with
# no old value (update_dpp(0, ..) cost a v_mov of 0 per neighbour) (MQ1)
VARS["MQ1"] = [
    ("""                const uint8_t *p43b = (const uint8_t *)T.p43s;""",
     """                const uint8_t *p43b = (const uint8_t *)T.p43s;
                uint32_t kfc = 0xFCu; /* in a VGPR: the scale address below is one v_and_or_b32 */
                __asm__ volatile("" : "+v"(kfc));"""),
    ("""                        const float sc = *(lds_cf32 *)(uintptr_t)(scb | (tv2 & 0xFCu));""",
     """                        const float sc = *(lds_cf32 *)(uintptr_t)(scb | (tv2 & kfc));"""),
    ("""                        const float sc = *(lds_cf32 *)(uintptr_t)(sc_base[c] | (tv2 & 0xFCu));""",
     """                        const float sc = *(lds_cf32 *)(uintptr_t)(sc_base[c] | (tv2 & kfc));"""),
    ("""                        up[k] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xf[17 - k]), 0x138, 0xF, 0xF, false));
                        dn[k] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xf[k]), 0x130, 0xF, 0xF, false));""",
     """                        up[k] = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(xf[17 - k]), 0x138, 0xF, 0xF, true));
                        dn[k] = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(xf[k]), 0x130, 0xF, 0xF, true));"""),
]

# k_huffman big_values rows stored 64 B (four groups) at a time: a lane completes half a line per
# store burst (ST64)
VARS["ST64"] = [
    ("""                    uint4 pend = make_uint4(0u, 0u, 0u, 0u);
                    bool held = false;""", """                    uint4 pend = make_uint4(0u, 0u, 0u, 0u), pend1 = pend, pend2 = pend;
                    int held = 0;"""),
    ("""                        const uint4 cur = make_uint4(wv[0], wv[1], wv[2], wv[3]);
                        if (held) { /* (k is uniform: no divergence) */
                            *(uint4 *)(row + k - 8) = pend;
                            *(uint4 *)(row + k) = cur;
                        } else {
                            pend = cur;
                        }
                        held = !held;""", """                        const uint4 cur = make_uint4(wv[0], wv[1], wv[2], wv[3]);
                        if (held == 3) { /* (k is uniform: no divergence) */
                            *(uint4 *)(row + k - 24) = pend;
                            *(uint4 *)(row + k - 16) = pend1;
                            *(uint4 *)(row + k - 8) = pend2;
                            *(uint4 *)(row + k) = cur;
                        } else if (held == 2) {
                            pend2 = cur;
                        } else if (held == 1) {
                            pend1 = cur;
                        } else {
                            pend = cur;
                        }
                        held = (held + 1) & 3;"""),
    ("""                    if (held) *(uint4 *)(row + k - 8) = pend; /* (before the count1 stores overwrite its tail) */""",
     """                    if (held == 3) {
                        *(uint4 *)(row + k - 24) = pend;
                        *(uint4 *)(row + k - 16) = pend1;
                        *(uint4 *)(row + k - 8) = pend2;
                    } else if (held == 2) {
                        *(uint4 *)(row + k - 16) = pend;
                        *(uint4 *)(row + k - 8) = pend1;
                    } else if (held == 1) {
                        *(uint4 *)(row + k - 8) = pend;
                    }"""),
]

# k_synth phase W: the shifted B pairs xbp[m] = (row 2m+1, row 2m+2) loaded by ds_read2_b32 straight
# into aligned register pairs (inline asm, three bases) -- the compiler paired the rows (2m, 2m+1)
# and shuffled them with 14 v_mov per granule (WXB)
VARS["WXB"] = [
    ("""#pragma unroll
                for (int m = 0; m < 8; m++) xbp[m] = (f32x2){sBuf[pb + (2 * m + 1) * XROW], sBuf[pb + (2 * m + 2) * XROW]};""",
     """                {
                    static_assert(XROW == 36, "WXB offsets");
                    const uint32_t ba = (uint32_t)(uintptr_t)(lds_cf32 *)&sBuf[pb];
                    const uint32_t bb = ba + 7u * 4u * XROW, bc2 = ba + 15u * 4u * XROW;
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:36 offset1:72" : "=v"(xbp[0]) : "v"(ba));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:108 offset1:144" : "=v"(xbp[1]) : "v"(ba));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:180 offset1:216" : "=v"(xbp[2]) : "v"(ba));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:0 offset1:36" : "=v"(xbp[3]) : "v"(bb));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:72 offset1:108" : "=v"(xbp[4]) : "v"(bb));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:144 offset1:180" : "=v"(xbp[5]) : "v"(bb));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:216 offset1:252" : "=v"(xbp[6]) : "v"(bb));
                    __asm__ volatile("ds_read2_b32 %0, %1 offset0:0 offset1:36" : "=v"(xbp[7]) : "v"(bc2));
                }"""),
    ("""                xb0 = sBuf[pb];
                xb17 = sBuf[pb + 17 * XROW];""",
     """                xb0 = sBuf[pb];
                xb17 = sBuf[pb + 17 * XROW];
                /* the asm loads land before any use: the wait carries them */
                __asm__ volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(xbp[0]), "+v"(xbp[1]), "+v"(xbp[2]), "+v"(xbp[3]), "+v"(xbp[4]), "+v"(xbp[5]),
                                   "+v"(xbp[6]), "+v"(xbp[7]));"""),
]

# timing probe (same output): per-phase shader-clock totals of one wave (block 0 / 4000, wave 0),
# printed at the stream's end (PHT)
VARS["PHT"] = [
    ("    float *const sBuf = Wd.buf;\n",
     "    float *const sBuf = Wd.buf;\n    unsigned long long ph_[4] = {0ull, 0ull, 0ull, 0ull}, tQ_ = 0ull, tI_ = 0ull, tM_ = 0ull, tW_ = 0ull;\n"),
    (_QS, "            tQ_ = clock64();\n" + _QS),
    (_IS, "            tI_ = clock64(); ph_[0] += tI_ - tQ_;\n" + _IS),
    (_MS, "            tM_ = clock64(); ph_[1] += tM_ - tI_;\n" + _MS),
    (_WS, "            tW_ = clock64(); ph_[2] += tW_ - tM_;\n" + _WS),
    ("            wave_sync(); /* X reads done before the next granule's xr */",
     "            wave_sync(); /* X reads done before the next granule's xr */\n            ph_[3] += clock64() - tW_;"),
    ("    if (f1 == F && PF != 1) {",
     "    if ((blockIdx.x == 0 || blockIdx.x == 4000) && threadIdx.x == 0 && !SRC_XR && !LSF)\n"
     "        printf(\"PHT blk %d Q %llu I %llu M %llu W %llu\\n\", (int)blockIdx.x, ph_[0], ph_[1], ph_[2], ph_[3]);\n"
     "    if (f1 == F && PF != 1) {"),
]

# PHT with phase Q split: Q1 band scales (to their wave_sync), Q2 requantise + stereo + scatter,
# Q3 xin + prefetch issue; G = end of W to the next Q (PHT2)
VARS["PHT2"] = [
    ("    float *const sBuf = Wd.buf;\n",
     "    float *const sBuf = Wd.buf;\n    unsigned long long ph_[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, tQ_ = 0ull, tI_ = 0ull, tM_ = 0ull, tW_ = 0ull, tE_ = 0ull, t1_ = 0ull, t2_ = 0ull;\n"),
    (_QS, "            tQ_ = clock64(); if (tE_) ph_[7] += tQ_ - tE_;\n" + _QS),
    ("                (void)m12a;\n", "                (void)m12a;\n                t1_ = clock64(); ph_[4] += t1_ - tQ_;\n"),
    ("                xin(xin_off);\n                } /* !fusedq */", "                t2_ = clock64(); ph_[5] += t2_ - t1_;\n                xin(xin_off);\n                } /* !fusedq */"),
    (_IS, "            tI_ = clock64(); ph_[0] += tI_ - tQ_; ph_[6] += tI_ - t2_;\n" + _IS),
    (_MS, "            tM_ = clock64(); ph_[1] += tM_ - tI_;\n" + _MS),
    (_WS, "            tW_ = clock64(); ph_[2] += tW_ - tM_;\n" + _WS),
    ("            wave_sync(); /* X reads done before the next granule's xr */",
     "            wave_sync(); /* X reads done before the next granule's xr */\n            tE_ = clock64(); ph_[3] += tE_ - tW_;"),
    ("    if (f1 == F && PF != 1) {",
     "    if ((blockIdx.x == 0 || blockIdx.x == 4000) && threadIdx.x == 0 && !SRC_XR && !LSF)\n"
     "        printf(\"PHT2 blk %d Q %llu (Q1 %llu Q2 %llu Q3 %llu) I %llu M %llu W %llu G %llu\\n\", (int)blockIdx.x, ph_[0], ph_[4], ph_[5], ph_[6], ph_[1], ph_[2], ph_[3], ph_[7]);\n"
     "    if (f1 == F && PF != 1) {"),
]

# PHT2 with Q2 split: Qa read_cis, Qb requant, Qc escape check + stereo, Qd scatter (PHT3)
VARS["PHT3"] = [
    ("    float *const sBuf = Wd.buf;\n",
     "    float *const sBuf = Wd.buf;\n    unsigned long long ph_[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, tQ_ = 0ull, t1_ = 0ull, ta_ = 0ull, tb_ = 0ull, tc_ = 0ull;\n"),
    ("                (void)m12a;\n", "                (void)m12a;\n                t1_ = clock64();\n"),
    ("                else read_cis(std::integral_constant<int, 5>{});\n",
     "                else read_cis(std::integral_constant<int, 5>{});\n                __asm__ volatile(\"s_waitcnt lgkmcnt(0)\" : \"+v\"(cis[0][0]), \"+v\"(cis[1][0]), \"+v\"(cis[0][1]), \"+v\"(cis[1][1]));\n                ta_ = clock64(); ph_[0] += ta_ - t1_;\n"),
    ("                else requant(std::integral_constant<int, 5>{});\n",
     "                else requant(std::integral_constant<int, 5>{});\n                __asm__ volatile(\"s_waitcnt lgkmcnt(0)\" : \"+v\"(xp[0][0]), \"+v\"(xp[1][0]));\n                tb_ = clock64(); ph_[1] += tb_ - ta_;\n"),
    ("                if (ms_fold) {\n",
     "                tc_ = clock64(); ph_[2] += tc_ - tb_;\n                if (ms_fold) {\n"),
    ("                xin(xin_off);\n                } /* !fusedq */", "                ph_[3] += clock64() - tc_;\n                xin(xin_off);\n                } /* !fusedq */"),
    ("    if (f1 == F && PF != 1) {",
     "    if ((blockIdx.x == 0 || blockIdx.x == 4000) && threadIdx.x == 0 && !SRC_XR && !LSF)\n"
     "        printf(\"PHT3 blk %d cis %llu requant %llu esc+stereo %llu scatter %llu\\n\", (int)blockIdx.x, ph_[0], ph_[1], ph_[2], ph_[3]);\n"
     "    if (f1 == F && PF != 1) {"),
]

# k_synth M/S scatter: chunks at or past nlive (all-zero lines) stored as zeros without the
# sum / difference (MSZ)
VARS["MSZ"] = [
    ("""                            scatter(i, 0, xp[0][i] + xp[1][i]);
                            scatter(i, 1, xp[0][i] - xp[1][i]);""",
     """                            if (i < 2 || i < nlive) {
                                scatter(i, 0, xp[0][i] + xp[1][i]);
                                scatter(i, 1, xp[0][i] - xp[1][i]);
                            } else {
                                scatter(i, 0, (f32x2){0.f, 0.f});
                                scatter(i, 1, (f32x2){0.f, 0.f});
                            }"""),
]

# k_synth phase M: the lane's S / X row offsets (two byte offsets, lane constants) computed once
# before the frame loop; the per-granule addresses are the wave's buffer base plus them, the row
# steps immediate offsets (MH)
VARS["MH"] = [
    ("    for (int f = fw; f < f1; f++) {\n        int nch, sr, mode = 0, mext = 0;",
     "    const int mlane_ = (int)(threadIdx.x & 63);\n"
     "    const uint32_t m_off_a = (uint32_t)(((mlane_ & 15) * SROW + 4 * (mlane_ >> 4)) * 4);\n"
     "    const uint32_t m_off_c = (uint32_t)((((mlane_ & 15) < 4 ? 32 + (mlane_ & 15) : 35) * SROW + 4 * (mlane_ >> 4)) * 4);\n"
     "    for (int f = fw; f < f1; f++) {\n        int nch, sr, mode = 0, mext = 0;"),
    ("""#pragma unroll
                for (int nt = 0; nt < 3; nt++) {
                    int n = 16 * nt + r16;
                    n = n < 36 ? n : 35;
                    const f32x4 a4 = *(const f32x4 *)&sBuf[n * SROW + 4 * q];
                    const f32x4 b4 = *(const f32x4 *)&sBuf[n * SROW + 16 + 4 * q]; /* S[31 - 4 q - ks] */""",
     """                typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
                const uint32_t sbase_ = (uint32_t)(uintptr_t)(lds_cf32 *)(const float *)sBuf;
                lds_f32x4 *const pA = (lds_f32x4 *)(uintptr_t)(sbase_ + m_off_a);
                lds_f32x4 *const pC = (lds_f32x4 *)(uintptr_t)(sbase_ + m_off_c);
#pragma unroll
                for (int nt = 0; nt < 3; nt++) {
                    lds_f32x4 *const pr = nt == 2 ? pC : pA + nt * (16 * SROW / 4);
                    const f32x4 a4 = pr[0];
                    const f32x4 b4 = pr[4]; /* S[31 - 4 q - ks] */"""),
    ("""#pragma unroll
                for (int nt = 0; nt < 3; nt++) {
                    const int n = 16 * nt + r16;
                    if (n < 36) {
                        *(f32x4 *)&sBuf[n * XROW + 4 * q] = ce[nt];
                        *(f32x4 *)&sBuf[n * XROW + 16 + 4 * q] = co[nt];
                    }
                }""",
     """                static_assert(XROW == SROW, "X rows reuse the S row offsets");
#pragma unroll
                for (int nt = 0; nt < 3; nt++) {
                    const int n = 16 * nt + r16;
                    if (n < 36) {
                        lds_f32x4 *const pr = nt == 2 ? pC : pA + nt * (16 * XROW / 4);
                        pr[0] = ce[nt];
                        pr[4] = co[nt];
                    }
                }"""),
]

# MH plus the S-row write offset and the A fragments' table offset hoisted the same way (MH2)
VARS["MH2"] = [
    (VARS["MH"][0][0], VARS["MH"][0][1].replace(
        "    for (int f = fw; f < f1; f++) {",
        "    const uint32_t m_off_s = (uint32_t)((18 * (mlane_ >> 5) * SROW + ((mlane_ & 31) < 16 ? (mlane_ & 31) : 47 - (mlane_ & 31))) * 4);\n"
        "    const uint32_t m_off_e = (uint32_t)(((mlane_ & 15) * 16 + 4 * (mlane_ >> 4)) * 4);\n"
        "    for (int f = fw; f < f1; f++) {")),
    ("""                const int sw = opaque(18 * ch * SROW + (sb < 16 ? sb : 47 - sb));
#pragma unroll
                for (int t = 0; t < 18; t++) sBuf[sw + t * SROW] = o18[t]; /* frequency inversion already in */""",
     """                typedef __attribute__((address_space(3))) float lds_f32;
                lds_f32 *const ps = (lds_f32 *)(uintptr_t)((uint32_t)(uintptr_t)(lds_cf32 *)(const float *)sBuf + m_off_s);
#pragma unroll
                for (int t = 0; t < 18; t++) ps[t * SROW] = o18[t]; /* frequency inversion already in */"""),
    ("""                const float4 ae = *(const float4 *)&T.ce[r16][4 * q];
                const float4 ao = *(const float4 *)&T.co[r16][4 * q];""",
     """                typedef __attribute__((address_space(3))) const f32x4 lds_cf4;
                const f32x4 ae = *(lds_cf4 *)(uintptr_t)((uint32_t)(uintptr_t)(lds_cf32 *)&T.ce[0][0] + m_off_e);
                const f32x4 ao = *(lds_cf4 *)(uintptr_t)((uint32_t)(uintptr_t)(lds_cf32 *)&T.co[0][0] + m_off_e);"""),
] + VARS["MH"][1:]

# xin from one lane-constant address (8 words below the lane's lines; held across the loop) with
# every read an immediate offset: the boundary subbands read a neighbour's words they do not use
# instead of selecting their own; a 256-B pad keeps wave 0's look-back inside the LDS object (XIN)
VARS["XIN"] = [
    ("""    struct Lds {
        SynWave Wv[SYN_WAVES];""", """    struct Lds {
        float pad_[64]; /* xin's look-back of wave 0, subband 0 (words it does not use) */
        SynWave Wv[SYN_WAVES];"""),
    ("    const int mlane_ = (int)(threadIdx.x & 63);\n",
     "    const int mlane_ = (int)(threadIdx.x & 63);\n"
     "    const uint32_t xin_off = (uint32_t)(((mlane_ >> 5) * 576 + 18 * (mlane_ & 31) - 8) * 4);\n"),
    ("""                const int lx = opaque((int)(threadIdx.x & 63));
                const int base = (lx >> 5) * 576 + 18 * (lx & 31), sbx = lx & 31;
#pragma unroll
                for (int i = 0; i < 9; i++) {
                    const float2 v = *(const float2 *)&sBuf[base + 2 * i];
                    xf[2 * i] = v.x;
                    xf[2 * i + 1] = v.y;
                }
                const int pb = sbx ? base - 8 : base, nb = sbx < 31 ? base + 18 : base;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float2 p = *(const float2 *)&sBuf[pb + 2 * i];
                    const float2 n = *(const float2 *)&sBuf[nb + 2 * i];""",
     """                typedef __attribute__((address_space(3))) const f32x2 lds_cf2;
                lds_cf2 *const P = (lds_cf2 *)(uintptr_t)((uint32_t)(uintptr_t)(lds_cf32 *)(const float *)sBuf + xin_off);
#pragma unroll
                for (int i = 0; i < 9; i++) {
                    const f32x2 v = P[4 + i];
                    xf[2 * i] = v.x;
                    xf[2 * i + 1] = v.y;
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const f32x2 p = P[i];
                    const f32x2 n = P[13 + i];"""),
]

# phase Q: the is[] words read right after the requantiser path is known, before the band scales,
# so their LDS latency overlaps the scales' chain (CISE)
VARS["CISE"] = [
    ("                fusedq = PAR && var[0] == 0 && var[1] == 0 && !is_on && !ms_fold;\n",
     "                fusedq = PAR && var[0] == 0 && var[1] == 0 && !is_on && !ms_fold;\n"
     "                if (!fusedq) {\n"
     "                    if (nlive == 2) read_cis(std::integral_constant<int, 2>{});\n"
     "                    else if (nlive == 3) read_cis(std::integral_constant<int, 3>{});\n"
     "                    else read_cis(std::integral_constant<int, 5>{});\n"
     "                }\n"),
    ("""                if (nlive == 2) read_cis(std::integral_constant<int, 2>{});
                else if (nlive == 3) read_cis(std::integral_constant<int, 3>{});
                else read_cis(std::integral_constant<int, 5>{});
                auto requant""", """                auto requant"""),
]

# phase W int16 stereo emit without the half-wave swap: each lane stores its own channel's two
# samples (2 B each; one instruction covers 128 contiguous bytes of L/R) (EMS)
VARS["EMS"] = [
    ("""                            const int vo = vo_st;
                            const int p0 = to_i32(o.x), p1 = to_i32(o.y);
                            const auto r = __builtin_amdgcn_permlane32_swap(p0, p1, false, false);
                            __builtin_amdgcn_raw_buffer_store_b32(
                                __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16((int)r[0], (int)r[1])), r_pcm,
                                vo + 256 * tp, so, 0);""",
     """                            const int vo = vo_st;
                            const uint32_t pk =
                                __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(to_i32(o.x), to_i32(o.y)));
                            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)pk, r_pcm, vo + 256 * tp, so, 0);
                            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(pk >> 16), r_pcm, vo + 256 * tp + 128, so, 0);"""),
    ("const int vo_st = opaque((sb + 32 * ch) * (F32 ? 8 : 4))",
     "const int vo_st = opaque(F32 ? (sb + 32 * ch) * 8 : (2 * sb + ch) * 2)"),
]

# phase Q's band scales: 2^((q & 3) / 4) by two independent selects instead of an LDS table read
# (one LDS round trip off the scales' chain) (P2S)
VARS["P2S"] = [
    ("                auto p2q = [&](int q) { return ldexpf(T.p2q[q & 3], q >> 2) * msf; };",
     """                auto p2q = [&](int q) {
                    const bool o = (q & 1) != 0;
                    const float lo = o ? 1.18920711500272106672f : 1.0f;
                    const float hi = o ? 1.68179283050742908606f : 1.41421356237309504880f;
                    return ldexpf((q & 2) ? hi : lo, q >> 2) * msf;
                };"""),
]

# more is[] row strides (int16 lines): 584 (+16 B), 592 (+32 B), 704 (+256 B) (ISR584 / ISR592 / ISR704)
VARS["ISR584"] = [("FLAGS", "-DMP3D_IS_ROW=584")]
VARS["ISR592"] = [("FLAGS", "-DMP3D_IS_ROW=592")]
VARS["ISR704"] = [("FLAGS", "-DMP3D_IS_ROW=704")]

# k_huffman work queue: the next round's ticket taken at the start of a round and its units'
# perm entries loaded right after this round's record loads, so neither latency sits between two
# rounds (TKP)
VARS["TKP"] = [
    ("""    for (;;) {
        uint32_t t = 0u;
        if (lane == 0) t = atomicAdd(work, 1u);
        const int ubase = 64 * (int)__builtin_amdgcn_readfirstlane(t);
        if (ubase >= n_units) break;
        {
            const int u = ubase + lane < n_units ? (int)perm[ubase + lane] : n_units;
            const int fr = u >> 2, gr = (u >> 1) & 1, ch = u & 1;
            bool valid = u < n_units;
            /* the stream's md base, loaded together with the frame record (not
             * after it: one memory latency less per round) */
            const uint64_t mdo = md_off[(valid ? fr : 0) / F];
            FrameRec r;
            uint64_t sq[4] = {0, 0, 0, 0};
            if (valid) {
                r = rec[fr];
                valid = r.frame_bytes && !(r.first_gr & (REC_TAG | REC_DROP)) && ch < r.nch && (gr == 0 || !r.lsf);
                const ulonglong2 a = *(const ulonglong2 *)&sideu[u & ~3];
                const ulonglong2 b = *(const ulonglong2 *)&sideu[(u & ~3) + 2];
                sq[0] = a.x; sq[1] = a.y; sq[2] = b.x; sq[3] = b.y;
            }""", """    uint32_t tk = 0u;
    if (lane == 0) tk = atomicAdd(work, 1u);
    int ubase = 64 * (int)__builtin_amdgcn_readfirstlane(tk);
    int u_pre = ubase + lane < n_units ? (int)perm[ubase + lane] : n_units;
    for (;;) {
        if (ubase >= n_units) break;
        {
            const int u = u_pre;
            /* the next round's ticket, issued before this round's loads */
            uint32_t tn = 0u;
            if (lane == 0) tn = atomicAdd(work, 1u);
            const int fr = u >> 2, gr = (u >> 1) & 1, ch = u & 1;
            bool valid = u < n_units;
            /* the stream's md base, loaded together with the frame record (not
             * after it: one memory latency less per round) */
            const uint64_t mdo = md_off[(valid ? fr : 0) / F];
            FrameRec r;
            uint64_t sq[4] = {0, 0, 0, 0};
            if (valid) {
                r = rec[fr];
                valid = r.frame_bytes && !(r.first_gr & (REC_TAG | REC_DROP)) && ch < r.nch && (gr == 0 || !r.lsf);
                const ulonglong2 a = *(const ulonglong2 *)&sideu[u & ~3];
                const ulonglong2 b = *(const ulonglong2 *)&sideu[(u & ~3) + 2];
                sq[0] = a.x; sq[1] = a.y; sq[2] = b.x; sq[3] = b.y;
            }
            /* ... and its units, in flight through this round (the barrier
             * keeps the ticket's wait after this round's record loads) */
            __asm__ volatile("" : "+v"(tn) : "v"(sq[0]), "v"(mdo));
            ubase = 64 * (int)__builtin_amdgcn_readfirstlane(tn);
            u_pre = ubase + lane < n_units ? (int)perm[ubase + lane] : n_units;"""),
]


# ---- round 6 bounds (timing only; output wrong by construction) ----
# NOIM: phase I without the fast 36-point IMDCT (its 18 inputs passed through
# as the DCT-IV outputs): the most any IMDCT speed-up (e.g. on the matrix
# cores) could take off k_synth
VARS["NOIM"] = [("""                    imdct36_wp(x, W, (const f32x2 *)(uintptr_t)(uint32_t)opaque((int)(uintptr_t)(lds_cf32 *)(const float *)&T.kc[0]));""",
                 """#pragma unroll
                    for (int n = 0; n < 9; n++) W[n] = (f32x2){x[n], x[17 - n]};""")]
# NOBS: phase Q without the band-scale step (lane = band: sf word by a
# cross-lane read, 2^(q/4), the LDS store and the wave sync after it) -- the
# scale rows keep whatever they held: the most a precomputed per-band scale
#  could take off
VARS["NOBS"] = [("""                    const float v = p2q(gain - ((sf + pre) << shift));
                    if (bl < 22) Wd.scale[c][bl] = v;""", """                    (void)gain; (void)shift; (void)wd; (void)sf; (void)pre; (void)bl;"""),
                ("""                wave_sync();
                (void)m12a;""", """                (void)m12a;""")]



# NOXIN: phase I's inputs not read back from the
# xr scatter (constants instead; the scatter stores stay): the most a
# register-only requantiser for M/S frames could save
VARS["NOXIN"] = [("""                    const f32x2 v = P[4 + i];
                    xf[2 * i] = v.x;""", """                    const f32x2 v = (f32x2){(float)i, 0.5f};
                    xf[2 * i] = v.x;"""),
                 ("""                    const f32x2 p = P[i];
                    const f32x2 n = P[13 + i];""", """                    const f32x2 p = (f32x2){0.25f, (float)i};
                    const f32x2 n = (f32x2){(float)i, 0.75f};""")]



# what in the band-scale step costs (NOBS took 9 % off k_synth):
# BSA: the compiler fence after the band scales dropped (the store -> read
#      order within the wave stays: LDS executes in order, and the scale reads'
#      addresses are integer-built, so the compiler keeps them after the
#      store) -- output unchanged
VARS["BSA"] = [("""                wave_sync();
                (void)m12a;""", """                (void)m12a;""")]
# BSB: the lane's scalefactor word from its own lane (no cross-lane read;
#      wrong scales, timing only)
VARS["BSB"] = [("""                    const uint32_t wd = (uint32_t)__shfl((int)wm[cs], c * MW + (j >> 2));
                    const int sf = (int)(wd >> (8 * (j & 3))) & 0xFF;
                    const int pre = (g11 & 0xFFu) ? (int)(MP3D_PRETAB_BITS >> (2 * j)) & 3 : 0;
                    const float v = p2q(gain - ((sf + pre) << shift));""",
                """                    const uint32_t wd = wm[cs];
                    const int sf = (int)(wd >> (8 * (j & 3))) & 0xFF;
                    const int pre = (g11 & 0xFFu) ? (int)(MP3D_PRETAB_BITS >> (2 * j)) & 3 : 0;
                    const float v = p2q(gain - ((sf + pre) << shift));""")]
# BSC: 2^((q & 3)/4) not read from the LDS table (1.0; wrong scales, timing only)
VARS["BSC"] = [("""                auto p2q = [&](int q) { return ldexpf(T.p2q[q & 3], q >> 2) * msf; };""",
                """                auto p2q = [&](int q) { return ldexpf(1.0f, q >> 2) * msf; };""")]



# HSTAT (round 6, VERDICT r05 item 4: account for k_huffman's reads): the
# staged main-data bytes of a launch and the distinct 128-B lines they span,
# counted by atomics (per lane: its segment's words and lines; plus one
# FrameRec + side-word line pair per frame), read back through an extra
# symbol of this build only (mp3d_dbg_hstat, abx/hstat.py).  Output unchanged.
VARS["HSTAT"] = [
    ("""            const uint32_t *src = (const uint32_t *)(md + (dec ? mdo : 0)) + w0;""",
     """            const uint32_t *src = (const uint32_t *)(md + (dec ? mdo : 0)) + w0;
            if (dec) {
                const uint64_t a0 = (uint64_t)(uintptr_t)src, a1 = a0 + 4ull * len;
                atomicAdd(&g_hstat[0], (unsigned long long)(4ull * len));
                atomicAdd(&g_hstat[1], (unsigned long long)(((a1 - 1) >> 7) - (a0 >> 7) + 1));
                atomicAdd(&g_hstat[2], 1ull);
            }"""),
    ("""/* k_huffman: one lane per unit (its layout constants and helpers: mp3d_huffman_dev.h) */""",
     """__device__ unsigned long long g_hstat[8];
/* k_huffman: one lane per unit (its layout constants and helpers: mp3d_huffman_dev.h) */"""),
    ("""    int n_units = n_streams * F * 4;
    if (wave) {""", """    int n_units = n_streams * F * 4;
    {
        static const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_hstat), z, sizeof(z), 0, hipMemcpyHostToDevice, strm);
    }
    if (wave) {"""),
    ("""                       n_units, F, work, (const uint32_t *)rank);
}

} // namespace mp3d
""", """                       n_units, F, work, (const uint32_t *)rank);
}

} // namespace mp3d
extern "C" __attribute__((visibility("default"))) int mp3d_dbg_hstat(unsigned long long *out8) {
    return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(mp3d::g_hstat), 8 * sizeof(unsigned long long), 0,
                                    hipMemcpyDeviceToHost);
}
"""),
]



# HSTAT2: HSTAT plus the bytes k_huffman's store instructions carry (every
# lane's big_values group stores, dead zero groups included, count1 stores,
# UnitMeta), one atomic per unit, into g_hstat[3]
VARS["HSTAT2"] = VARS["HSTAT"] + [
    ("""                    uint4 pend[HUFF_BURST - 1];""", """                    uint4 pend[HUFF_BURST - 1];
                    unsigned long long st_bytes = 56ull; /* UnitMeta: sf 40 B + 16 B */"""),
    ("""                        const int slot = (k >> 3) % HUFF_BURST; /* (k is uniform: no divergence) */""",
     """                        st_bytes += 16ull;
                        const int slot = (k >> 3) % HUFF_BURST; /* (k is uniform: no divergence) */"""),
    ("""                        if (!two) {
                            c1_store(k, se0);""", """                        if (!two) {
                            st_bytes += 8ull;
                            c1_store(k, se0);"""),
    ("""                        __builtin_memcpy(row + k, &q, 16);
                        k += 8;
                    }""", """                        __builtin_memcpy(row + k, &q, 16);
                        st_bytes += 16ull;
                        k += 8;
                    }
                    atomicAdd(&g_hstat[3], st_bytes);"""),
]



# WPRE (timing only; wrong decode): the big_values loop's window words read
# at the PREVIOUS pair's position, one pair ahead, so the window load is off
# the pair-to-pair dependency chain (the funnel shift still uses the current
# position): the most a register-resident bit buffer could take off k_huffman
VARS["WPRE"] = [
    ("""                    uint4 pend[HUFF_BURST - 1];""", """                    uint4 pend[HUFF_BURST - 1];
                    uint32_t pw0, pw1, pw2;
                    {
                        const uint32_t w = (pos + 31u) >> 5;
                        pw0 = bits[(int)w - 1]; pw1 = bits[w]; pw2 = bits[w + 1];
                    }"""),
    ("""                            uint32_t hi, lo;
                            win64g(bits, pos, hi, lo);""", """                            uint32_t hi, lo;
                            hi = __builtin_amdgcn_alignbit(pw0, pw1, 0u - pos);
                            lo = __builtin_amdgcn_alignbit(pw1, pw2, 0u - pos);
                            {
                                const uint32_t w = (pos + 31u) >> 5;
                                pw0 = bits[(int)w - 1]; pw1 = bits[w]; pw2 = bits[w + 1];
                            }"""),
]



# HSTAT3: HSTAT2 plus the staging batches: g_hstat[4] += batches of a round
# (the while loop's passes), g_hstat[5] += rounds, g_hstat[6] += lanes that
# did not fit the first batch
VARS["HSTAT3"] = [(a.replace("g_hstat[4]", "g_hstat[8]"), b.replace("g_hstat[4]", "g_hstat[8]"))
                  for a, b in VARS["HSTAT2"]] + [
    ("""            bool pending = dec;
            while (__ballot(pending)) {""", """            bool pending = dec;
            int nbatch = 0;
            while (__ballot(pending)) {
                nbatch++;"""),
    ("""                pending = pending && !inb;
            }""", """                pending = pending && !inb;
                if (nbatch == 1 && pending) atomicAdd(&g_hstat[6], 1ull);
            }
            if (lane == 0) {
                atomicAdd(&g_hstat[4], (unsigned long long)nbatch);
                atomicAdd(&g_hstat[5], 1ull);
            }"""),
]



# NO2B (timing only; 4 % of C3's units not decoded): k_huffman's rounds decode
# their first staging batch only -- what the second batches (1.26 per round
# on C3 after the scfsi pieces) cost
VARS["NO2B"] = [("""                pending = pending && !inb;
            }
            if (valid && !dec) {""", """                pending = false;
            }
            if (valid && !dec) {""")]


if __name__ == "__main__":
    for n in (sys.argv[1:] or VARS):
        variant(n, VARS[n])
