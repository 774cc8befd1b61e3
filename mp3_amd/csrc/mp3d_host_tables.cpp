/*
 * mp3d_host_tables.cpp -- constant-table construction (ISO 11172-3 Annex B
 * and 2.4.3.4 formulas) and the one-time upload per device.
 */
#include <mutex>

#include "mp3d_host.h"
#include "mp3d_consts.h"

using namespace mp3d;

static void build_huffman_lut(DevTables &t) {
    /* two-level LUT: first level min(8, maxlen) bits; codes longer than that
     * go through one sub-table per first-level prefix (mp3d_internal.h) */
    std::vector<uint16_t> lut;
    const uint16_t UNUSED = 0xFFFF;
    for (int ti = 0; ti < MP3D_LUT_TABLES; ti++) {
        std::vector<uint32_t> code, len, val;
        if (ti < MP3D_NUM_HTABS) {
            int n = MP3D_HTAB_ROWLEN[ti];
            for (int x = 0; x < n; x++)
                for (int y = 0; y < n; y++) {
                    code.push_back(MP3D_HTAB_CODES[ti][x * n + y]);
                    len.push_back(MP3D_HTAB_LENS[ti][x * n + y]);
                    val.push_back((uint32_t)(x << 4 | y));
                }
        } else {
            for (int v = 0; v < 16; v++) {
                code.push_back(MP3D_QUAD_CODE[0][v]);
                len.push_back(MP3D_QUAD_LEN[0][v]);
                val.push_back((uint32_t)v);
            }
        }
        uint32_t maxlen = *std::max_element(len.begin(), len.end());
        int b1 = (int)std::min<uint32_t>(8, maxlen);
        if (lut.size() & 1) lut.push_back(UNUSED);
        size_t base = lut.size();
        t.lut_hdr.base[ti] = (uint16_t)base;
        t.lut_hdr.bits1[ti] = (uint8_t)b1;
        lut.resize(base + (1u << b1), UNUSED);
        std::vector<int> subbits(1u << b1, 0);
        for (size_t i = 0; i < code.size(); i++)
            if ((int)len[i] > b1) {
                uint32_t p = code[i] >> (len[i] - b1);
                subbits[p] = std::max(subbits[p], (int)len[i] - b1);
            }
        std::vector<size_t> subbase(1u << b1, 0);
        for (uint32_t p = 0; p < (1u << b1); p++)
            if (subbits[p]) {
                while (lut.size() & 3) lut.push_back(UNUSED); /* sub-tables 4-entry aligned */
                const size_t abs4 = lut.size() / 4;
                if (abs4 > 0x7FF || subbits[p] > 15) {
                    fprintf(stderr, "mp3d: LUT pointer overflow\n");
                    abort();
                }
                subbase[p] = lut.size();
                lut.resize(lut.size() + (1u << subbits[p]), UNUSED);
                lut[base + p] = (uint16_t)(0x8000u | ((uint32_t)subbits[p] << 11) | (uint32_t)abs4);
            }
        for (size_t i = 0; i < code.size(); i++) {
            /* big_values leaves: bits 13 / 14 flag x != 0 / y != 0 (a sign bit follows) */
            const uint32_t sgn = ti < MP3D_NUM_HTABS ? ((val[i] >> 4) != 0) << 13 | ((val[i] & 15) != 0) << 14 : 0u;
            uint16_t leaf = (uint16_t)((len[i] << 8) | val[i] | sgn);
            if ((int)len[i] <= b1) {
                uint32_t first = code[i] << (b1 - len[i]), cnt = 1u << (b1 - len[i]);
                for (uint32_t k = 0; k < cnt; k++) lut[base + first + k] = leaf;
            } else {
                uint32_t p = code[i] >> (len[i] - b1);
                int nb = subbits[p];
                uint32_t rest = code[i] & ((1u << (len[i] - b1)) - 1);
                uint32_t first = rest << (nb - (len[i] - b1)), cnt = 1u << (nb - (len[i] - b1));
                for (uint32_t k = 0; k < cnt; k++) lut[subbase[p] + first + k] = leaf;
            }
        }
    }
    if (lut.size() > MP3D_LUT_MAX) {
        fprintf(stderr, "mp3d: LUT overflow %zu\n", lut.size());
        abort();
    }
    for (size_t i = 0; i < lut.size(); i++) t.lut[i] = lut[i] == UNUSED ? (uint16_t)(1u << 8) : lut[i];
    /* table_select 0, 4, 14: a 2-entry all-zero table (zero-length leaves)
     * right after the last table (t.lut is zeroed past lut.size()) */
    const size_t zbase = (lut.size() + 1) & ~(size_t)1;
    if (zbase + 2 + 16 > MP3D_LUT_MAX) { /* + count1 table B in k_huffman's LDS copy */
        fprintf(stderr, "mp3d: LUT overflow %zu\n", zbase + 2);
        abort();
    }
    for (int i = 0; i < 32; i++) {
        const int ti = MP3D_HTAB_OF_SELECT[i];
        t.tsel[i] = ti < 0 ? (uint32_t)zbase | (1u << 16) | (1u << 20)
                           : (uint32_t)t.lut_hdr.base[ti] | ((uint32_t)t.lut_hdr.bits1[ti] << 16) |
                                 ((uint32_t)MP3D_LINBITS[i] << 24);
    }
    for (int sr = 0; sr < 9; sr++) {
        int acc = 0;
        for (int b = 0; b < 22; b++) {
            t.lbnd[sr][b] = (uint16_t)acc;
            acc += MP3D_SFB_LONG_WIDTH[sr][b];
        }
        t.lbnd[sr][22] = (uint16_t)acc;
    }
}

static_assert(offsetof(DevTables, lut) % 16 == 0, "k_huffman stages the LUT in 16-B loads");
static void build_tables(DevTables &t) {
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < 8208; i++) t.pow43[i] = (float)pow((double)i, 4.0 / 3.0);
    for (int m = 0; m < 32; m++)
        for (int k = 0; k < 32; k++) t.dct_c[m][k] = (float)cos(m * (2 * k + 1) * M_PI / 64.0);
    double D[512];
    for (int i = 0; i <= 256; i++) {
        double v = MP3D_SYNTH_WINDOW_Q16[i] / 65536.0;
        D[i] = v;
        if (i > 0) D[512 - i] = (i % 64) ? -v : v;
    }
    for (int j = 0; j < 32; j++) {
        int a, sa, b, sbn = -1;
        if (j < 16) { a = 16 + j; sa = 1; b = 16 - j; }
        else if (j == 16) { a = 0; sa = 0; b = 0; }
        else { a = 48 - j; sa = -1; b = j - 16; }
        t.win_a[j] = (uint8_t)a;
        t.win_b[j] = (uint8_t)b;
        for (int i = 0; i < 8; i++) {
            t.dwin[j][2 * i] = (float)(sa * D[64 * i + j]);
            t.dwin[j][2 * i + 1] = (float)(sbn * D[64 * i + 32 + j]);
        }
    }
    for (int sr = 0; sr < 9; sr++) {
        /* mixed blocks: long bands below line 36 (72 at MPEG-2.5 8 kHz, whose
         * bands are twice as wide): 8 MPEG-1 bands, 6 LSF bands (FFmpeg) */
        const int mix_end = sr == 8 ? 72 : 36;
        int lb[576], sidx[576], sdst[576];
        int l = 0;
        for (int b = 0; b < 22; b++)
            for (int n = 0; n < MP3D_SFB_LONG_WIDTH[sr][b]; n++) lb[l++] = b;
        int p = 0;
        for (int b = 0; b < 13; b++) {
            int w = MP3D_SFB_SHORT_WIDTH[sr][b];
            for (int off = 0; off < 3 * w; off++) {
                int win = off / w, f = off % w;
                sidx[p + off] = 22 + 3 * b + win;
                sdst[p + off] = p + 3 * f + win;
            }
            p += 3 * w;
        }
        for (int k = 0; k < 288; k++) {
            for (int v = 0; v < 3; v++) {
                int band[2], pos[2];
                for (int e = 0; e < 2; e++) {
                    const int i = 2 * k + e;
                    const bool lng = v == 0 || (v == 2 && i < mix_end);
                    band[e] = lng ? lb[i] : sidx[i];
                    pos[e] = lng ? i : sdst[i];
                }
                if (band[0] != band[1]) abort(); /* odd band width: impossible (ISO tables) */
                t.lpair[sr][v][k] = (uint32_t)(4 * band[0]) | (uint32_t)pos[0] << 8 | (uint32_t)pos[1] << 18;
            }
        }
    }
    build_huffman_lut(t);
}

static int upload_symbols() {
    float imdct12[6][6], win36[4][36], win12[12], cs[8], ca[8], isr[7][2], p2q[4], isl[2][16][2];
    for (int k = 0; k < 6; k++)
        for (int o = 0; o < 6; o++) {
            int i = o < 3 ? o : 6 + (o - 3);
            imdct12[k][o] = (float)cos(M_PI / 24.0 * (2 * i + 7) * (2 * k + 1));
        }
    /* long windows (block types 0, 1, 3) with the fast IMDCT's output
     * scale s_n = 1 / (2 cos(pi (2n+1) / 72)) and signs folded in
     * (mp3d_synth.hip imdct36_w): out i<9 uses y_(9+i), i in 9..17 -y_(26-i),
     * 18..26 -y_(26-i), 27..35 -y_(i-27)                                   */
    for (int bt = 0; bt < 4; bt++)
        for (int i = 0; i < 36; i++) {
            double w;
            if (bt == 0 || bt == 2) w = sin(M_PI / 36.0 * (i + 0.5));
            else if (bt == 1) w = i < 18 ? sin(M_PI / 36.0 * (i + 0.5)) : i < 24 ? 1.0 : i < 30 ? sin(M_PI / 12.0 * (i - 18 + 0.5)) : 0.0;
            else w = i < 6 ? 0.0 : i < 12 ? sin(M_PI / 12.0 * (i - 6 + 0.5)) : i < 18 ? 1.0 : sin(M_PI / 36.0 * (i + 0.5));
            int n = i < 9 ? 9 + i : i < 27 ? 26 - i : i - 27;
            double sc = 1.0 / (2.0 * cos(M_PI * (2 * n + 1) / 72.0));
            win36[bt][i] = (float)((i < 9 ? 1.0 : -1.0) * w * sc);
        }
    for (int i = 0; i < 12; i++) win12[i] = (float)sin(M_PI / 12.0 * (i + 0.5));
    for (int i = 0; i < 8; i++) {
        double c = MP3D_ALIAS_C[i], d = sqrt(1.0 + c * c);
        cs[i] = (float)(1.0 / d);
        ca[i] = (float)(c / d);
    }
    for (int p = 0; p < 7; p++) {
        if (p == 6) { isr[p][0] = 1.f; isr[p][1] = 0.f; continue; }
        double tn = tan(p * M_PI / 12.0);
        isr[p][0] = (float)(tn / (1.0 + tn));
        isr[p][1] = (float)(1.0 / (1.0 + tn));
    }
    /* LSF intensity (13818-3 2.4.3.2; FFmpeg is_table_lsf): is_pos p with
     * intensity_scale j -> (2^(-(j+1) ((p+1)/2) / 4), 1) for odd p, swapped
     * for even p (L = x * [0], R = x * [1]) */
    for (int j = 0; j < 2; j++)
        for (int p = 0; p < 16; p++) {
            const float f = (float)pow(2.0, -(j + 1) * ((p + 1) >> 1) / 4.0);
            isl[j][p][0] = (p & 1) ? f : 1.f;
            isl[j][p][1] = (p & 1) ? 1.f : f;
        }
    for (int i = 0; i < 4; i++) p2q[i] = (float)pow(2.0, i / 4.0);
    for (int i = 0; i < 22; i++)
        if (((MP3D_PRETAB_BITS >> (2 * i)) & 3u) != MP3D_PRETAB[i]) return MP3D_E_ARG; /* table drift */
    /* the kernel's literal tables (mp3d_consts.h, tools/gen_consts.py) must
     * equal this recipe bit for bit */
    for (int k = 0; k < 6; k++)
        for (int o = 0; o < 6; o++)
            if (imdct12[k][o] != MP3D_K_IMDCT12[k][o]) return MP3D_E_ARG;
    for (int i = 0; i < 12; i++)
        if (win12[i] != MP3D_K_WIN12[i]) return MP3D_E_ARG;
    for (int i = 0; i < 8; i++)
        if (cs[i] != MP3D_K_ALIAS_CS[i] || ca[i] != MP3D_K_ALIAS_CA[i]) return MP3D_E_ARG;
    uint16_t fbt[9][16] = {};
    for (int sr = 0; sr < 9; sr++)
        for (int bi = 1; bi < 15; bi++)
            fbt[sr][bi] = (uint16_t)((sr < 3 ? 144000 * (int)MP3D_BITRATE_L3[bi] : 72000 * (int)MP3D_BITRATE_L3_LSF[bi]) /
                                     (int)MP3D_SAMPLE_RATE[sr]);
    HIPCHK(upload_synth_constants(&win36[0][0], &isr[0][0], p2q, &isl[0][0][0]));
    HIPCHK(upload_demux_constants(&fbt[0][0]));
    HIPCHK(upload_frame_constants(&fbt[0][0]));
    return MP3D_OK;
}

static std::mutex g_mu;
DeviceCtx mp3d::g_dev[64];

int mp3d::device_init(int device) {
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MP3D_E_NO_DEVICE;
    if (device < 0 || device >= n || device >= 64) return MP3D_E_NO_DEVICE;
    DeviceCtx &c = g_dev[device];
    HIPCHK(hipSetDevice(device));
    if (c.ready) return MP3D_OK;
    int r = upload_symbols();
    if (r) return r;
    static DevTables host_tables;
    static bool built = false;
    if (!built) {
        build_tables(host_tables);
        built = true;
    }
    HIPCHK(hipMalloc(&c.tables, sizeof(DevTables)));
    HIPCHK(hipMemcpy(c.tables, &host_tables, sizeof(DevTables), hipMemcpyHostToDevice));
    /* the uploads above run on the null stream, and every handle's kernels
     * on non-blocking streams, which do not order after it: complete them
     * here, once per device */
    HIPCHK(hipDeviceSynchronize());
    (void)hipDeviceGetAttribute(&c.n_cu, hipDeviceAttributeMultiprocessorCount, device);
    c.ready = true;
    return MP3D_OK;
}
