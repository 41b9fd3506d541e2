// Baseline JPEG on the host: a bounded parser and Huffman (entropy) decoder, and below them the entropy ENCODER with the quality
// tables and the stream header.  Plain C++, no HIP: dgp_jpeg.hip includes it for the C-ABI's dgp_jpeg_probe / dgp_jpeg_entropy_decode /
// dgp_jpeg_entropy_encode, and stand-alone programs (tests/jpeg_host_main.cpp, tests/jpeg_enc_host_main.cpp) include it on their own.
//
// Written from ITU-T T.81: marker segments (B.2), Huffman table generation (Annex C), the decode procedures (F.2.2), the typical
// tables of Annex K.3 for streams that carry none (plain MJPEG frames).  Only SOF0 in one interleaved scan is accepted.  No globals,
// no allocation: every call works on its arguments and its own stack, so any number of threads may decode at once.
//
// Safety: every read of `data` goes through an index checked against `n`, every coefficient block address is derived from the geometry
// that was checked against the caller's dgp_jpeg_info, and a malformed stream ends in an error string, never in an out-of-range access.
#ifndef DGP_JPEG_HOST_H
#define DGP_JPEG_HOST_H

#include "../../include/dgp_hip.h"

#include <stdint.h>
#include <string.h>

namespace dgp_jpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3: table counts per code length 1..16, then the symbols
static const uint8_t kStdDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kStdDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kStdDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kStdAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
static const uint8_t kStdAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static const uint8_t kStdAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
static const uint8_t kStdAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// The block geometry of a frame of H x W with `sampling`: what the parser, the entropy decoder and the device launcher all use.
// Component c has its blocks on a grid of blocks_y[c] x blocks_x[c] (MCU-padded); luma sampling factors are (hs, vs), chroma 1 x 1.
static inline bool geometry(int32_t W, int32_t H, int32_t sampling, dgp_jpeg_info* g) {
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < DGP_JPEG_GRAY || sampling > DGP_JPEG_420) return false;
    const int hs = (sampling == DGP_JPEG_422 || sampling == DGP_JPEG_420) ? 2 : 1, vs = sampling == DGP_JPEG_420 ? 2 : 1;
    memset(g, 0, sizeof(*g));
    g->width = W;
    g->height = H;
    g->ncomp = sampling == DGP_JPEG_GRAY ? 1 : 3;
    g->sampling = sampling;
    g->mcus_x = (W + 8 * hs - 1) / (8 * hs);
    g->mcus_y = (H + 8 * vs - 1) / (8 * vs);
    g->total_blocks = 0;
    for (int c = 0; c < g->ncomp; ++c) {
        g->blocks_x[c] = g->mcus_x * (c == 0 ? hs : 1);
        g->blocks_y[c] = g->mcus_y * (c == 0 ? vs : 1);
        g->blocks[c] = g->blocks_x[c] * g->blocks_y[c];
        g->total_blocks += g->blocks[c];      // at most 3 * 8192^2: fits int32
    }
    return true;
}

struct Huff {
    uint8_t look_len[512];      // code length of the code a 9-bit prefix starts with (0: longer than 9 bits)
    uint8_t look_sym[512];
    int32_t maxcode[17];        // largest code of length l, -1 when there is none
    int32_t valoff[17];         // index of the first symbol of length l minus its first code
    uint8_t vals[256];
    bool present;
};

// Annex C: canonical codes from the counts; false when the counts do not describe a prefix code
static inline bool build_huff(Huff* h, const uint8_t* bits, const uint8_t* vals, int nvals) {
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    if (total != nvals || total > 256) return false;
    memcpy(h->vals, vals, (size_t)nvals);
    memset(h->look_len, 0, sizeof(h->look_len));
    memset(h->look_sym, 0, sizeof(h->look_sym));
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = bits[l - 1];
        h->valoff[l] = k - code;
        if (code + cnt > (1 << l)) return false;
        for (int i = 0; i < cnt; ++i, ++k, ++code)
            if (l <= 9) {
                const int first = code << (9 - l);
                for (int f = 0; f < (1 << (9 - l)); ++f) {
                    h->look_len[first + f] = (uint8_t)l;
                    h->look_sym[first + f] = vals[k];
                }
            }
        h->maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    h->present = true;
    return true;
}

struct State {
    dgp_jpeg_info info;
    uint16_t qt[4][64];         // natural order
    bool qt_ok[4];
    Huff dc[4], ac[4];
    int tq[3], td[3], ta[3];
};

static inline bool err(const char** why, const char* msg) {
    if (why) *why = msg;
    return false;
}

// Parses the marker segments up to and including the one SOS header.  Fills s->info (scan_offset = first entropy-coded byte).
static inline bool parse(const uint8_t* d, int64_t n, State* s, const char** why) {
    if (!d || n < 4) return err(why, "jpeg: no data");
    if (d[0] != 0xFF || d[1] != 0xD8) return err(why, "jpeg: no SOI marker");
    memset(s->qt_ok, 0, sizeof(s->qt_ok));
    for (int i = 0; i < 4; ++i) s->dc[i].present = s->ac[i].present = false;
    bool have_sof = false, saw_jfif = false, saw_adobe = false;
    int adobe_transform = 0, restart = 0, sampling = -1, W = 0, H = 0, ncomp = 0;
    int comp_id[3] = {0, 0, 0};
    int64_t p = 2;
    for (;;) {
        if (p + 2 > n) return err(why, "jpeg: truncated before the scan");
        if (d[p] != 0xFF) return err(why, "jpeg: marker expected");
        while (p + 1 < n && d[p + 1] == 0xFF) ++p;      // fill bytes
        if (p + 2 > n) return err(why, "jpeg: truncated before the scan");
        const int m = d[p + 1];
        p += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // parameterless
        if (m == 0xD9) return err(why, "jpeg: EOI before any scan");
        if (p + 2 > n) return err(why, "jpeg: truncated segment");
        const int64_t L = ((int64_t)d[p] << 8) | d[p + 1];
        if (L < 2 || p + L > n) return err(why, "jpeg: truncated segment");
        const int64_t q = p + 2, e = p + L;                      // payload [q, e)
        if (m == 0xC0) {
            if (have_sof) return err(why, "jpeg: two frame headers");
            if (e - q < 6) return err(why, "jpeg: short SOF0");
            if (d[q] != 8) return err(why, "jpeg: sample precision is not 8 bits");
            H = (d[q + 1] << 8) | d[q + 2];
            W = (d[q + 3] << 8) | d[q + 4];
            ncomp = d[q + 5];
            if (ncomp == 4) return err(why, "jpeg: 4 components (CMYK / YCCK) are not supported");
            if (ncomp != 1 && ncomp != 3) return err(why, "jpeg: 1 or 3 components expected");
            if (H == 0 || W == 0) return err(why, "jpeg: empty image");
            if (e - q != 6 + 3 * ncomp) return err(why, "jpeg: inconsistent SOF0 length");
            int hv[3] = {0, 0, 0};
            for (int c = 0; c < ncomp; ++c) {
                comp_id[c] = d[q + 6 + 3 * c];
                hv[c] = d[q + 7 + 3 * c];
                s->tq[c] = d[q + 8 + 3 * c];
                if (s->tq[c] > 3) return err(why, "jpeg: quantisation table id above 3");
            }
            if (ncomp == 1) {
                if ((hv[0] >> 4) < 1 || (hv[0] >> 4) > 4 || (hv[0] & 15) < 1 || (hv[0] & 15) > 4) return err(why, "jpeg: bad sampling factors");
                sampling = DGP_JPEG_GRAY;          // one component: its scan is not interleaved, whatever the factors say
            } else {
                if (hv[1] != 0x11 || hv[2] != 0x11) return err(why, "jpeg: unsupported chroma sampling (only 4:4:4, 4:2:2 h2v1, 4:2:0)");
                sampling = hv[0] == 0x11 ? DGP_JPEG_444 : hv[0] == 0x21 ? DGP_JPEG_422 : hv[0] == 0x22 ? DGP_JPEG_420 : -1;
                if (sampling < 0) return err(why, "jpeg: unsupported chroma sampling (only 4:4:4, 4:2:2 h2v1, 4:2:0)");
                if (comp_id[0] == comp_id[1] || comp_id[0] == comp_id[2] || comp_id[1] == comp_id[2]) return err(why, "jpeg: duplicate component ids");
            }
            have_sof = true;
        } else if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) {
            return err(why, "jpeg: progressive streams are not supported (baseline SOF0 only)");
        } else if (m >= 0xC9 && m <= 0xCF && m != 0xCC) {
            return err(why, "jpeg: arithmetic-coded streams are not supported (baseline SOF0 only)");
        } else if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC7 || m == 0xC8) {
            return err(why, "jpeg: only baseline SOF0 streams are supported");
        } else if (m == 0xCC) {
            return err(why, "jpeg: arithmetic-coded streams are not supported (baseline SOF0 only)");
        } else if (m == 0xC4) {
            int64_t t = q;
            while (t < e) {
                if (e - t < 17) return err(why, "jpeg: truncated DHT");
                const int tc = d[t] >> 4, th = d[t] & 15;
                if (tc > 1 || th > 3) return err(why, "jpeg: bad Huffman table id");
                int nv = 0;
                for (int l = 0; l < 16; ++l) nv += d[t + 1 + l];
                if (nv > 256 || e - t < 17 + nv) return err(why, "jpeg: truncated DHT");
                if (!build_huff(tc ? &s->ac[th] : &s->dc[th], d + t + 1, d + t + 17, nv)) return err(why, "jpeg: Huffman table is no prefix code");
                t += 17 + nv;
            }
        } else if (m == 0xDB) {
            int64_t t = q;
            while (t < e) {
                const int pq = d[t] >> 4, tqid = d[t] & 15;
                if (pq != 0) return err(why, "jpeg: 16-bit quantisation tables are not supported");
                if (tqid > 3) return err(why, "jpeg: quantisation table id above 3");
                if (e - t < 65) return err(why, "jpeg: truncated DQT");
                for (int k = 0; k < 64; ++k) s->qt[tqid][kZigzag[k]] = d[t + 1 + k];
                s->qt_ok[tqid] = true;
                t += 65;
            }
        } else if (m == 0xDD) {
            if (L != 4) return err(why, "jpeg: bad DRI length");
            restart = (d[q] << 8) | d[q + 1];
        } else if (m == 0xE0) {
            if (e - q >= 5 && d[q] == 'J' && d[q + 1] == 'F' && d[q + 2] == 'I' && d[q + 3] == 'F' && d[q + 4] == 0) saw_jfif = true;
        } else if (m == 0xEE) {
            if (e - q >= 12 && d[q] == 'A' && d[q + 1] == 'd' && d[q + 2] == 'o' && d[q + 3] == 'b' && d[q + 4] == 'e') {
                saw_adobe = true;
                adobe_transform = d[q + 11];
            }
        } else if (m == 0xDC) {
            return err(why, "jpeg: DNL is not supported");
        } else if (m == 0xDA) {
            if (!have_sof) return err(why, "jpeg: scan before the frame header");
            if (e - q < 1) return err(why, "jpeg: short SOS");
            const int ns = d[q];
            if (ns != ncomp) return err(why, "jpeg: several scans (one interleaved scan expected)");
            if (e - q != 4 + 2 * ns) return err(why, "jpeg: inconsistent SOS length");
            for (int c = 0; c < ns; ++c) {
                if (d[q + 1 + 2 * c] != comp_id[c]) return err(why, "jpeg: scan components do not follow the frame header");
                s->td[c] = d[q + 2 + 2 * c] >> 4;
                s->ta[c] = d[q + 2 + 2 * c] & 15;
                if (s->td[c] > 3 || s->ta[c] > 3) return err(why, "jpeg: bad Huffman table id");
            }
            if (d[q + 1 + 2 * ns] != 0 || d[q + 2 + 2 * ns] != 63 || d[q + 3 + 2 * ns] != 0)
                return err(why, "jpeg: spectral selection / successive approximation in a baseline scan");
            p = e;
            break;
        }
        p = e;                                                   // (APPn, COM and unknown segments are skipped)
    }
    if (ncomp == 3) {
        // the colour space libjpeg would assume: JFIF says YCbCr; else Adobe's transform flag; else component ids R, G, B mean RGB
        if (saw_adobe && adobe_transform != 1) return err(why, "jpeg: Adobe APP14 transform is not YCbCr");
        if (!saw_jfif && !saw_adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
            return err(why, "jpeg: RGB components, not YCbCr");
    }
    // slots 0 and 1 without a DHT get the typical tables (plain MJPEG frames carry none)
    if (!s->dc[0].present) build_huff(&s->dc[0], kStdDcLumBits, kStdDcVals, 12);
    if (!s->dc[1].present) build_huff(&s->dc[1], kStdDcChrBits, kStdDcVals, 12);
    if (!s->ac[0].present) build_huff(&s->ac[0], kStdAcLumBits, kStdAcLumVals, 162);
    if (!s->ac[1].present) build_huff(&s->ac[1], kStdAcChrBits, kStdAcChrVals, 162);
    for (int c = 0; c < ncomp; ++c) {
        if (!s->qt_ok[s->tq[c]]) return err(why, "jpeg: a component names a quantisation table that was not defined");
        if (!s->dc[s->td[c]].present || !s->ac[s->ta[c]].present) return err(why, "jpeg: a component names a Huffman table that was not defined");
    }
    if (!geometry(W, H, sampling, &s->info)) return err(why, "jpeg: bad geometry");
    s->info.restart_interval = restart;
    s->info.scan_offset = p;
    return true;
}

struct Bits {
    const uint8_t* d;
    int64_t pos, n;
    uint64_t acc;
    int nbits;

    // whole bytes into the accumulator; FF 00 is a data byte FF, FF followed by anything else is a marker and ends the data
    inline void refill() {
        while (nbits <= 56 && pos < n) {
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || d[pos + 1] != 0) return;
                pos += 2;
            } else {
                pos += 1;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    inline uint32_t peek16() {
        if (nbits < 16) refill();
        return (uint32_t)(nbits >= 16 ? (acc >> (nbits - 16)) : (acc << (16 - nbits))) & 0xFFFFu;      // (short of data: zero-padded)
    }
    inline bool take(int k, int32_t* v) {      // 1 <= k <= 16
        if (nbits < k) {
            refill();
            if (nbits < k) return false;
        }
        *v = (int32_t)((acc >> (nbits - k)) & ((1u << k) - 1u));
        nbits -= k;
        return true;
    }
};

// F.2.2.3: one symbol; -1 = no code of 16 bits or fewer matches, -2 = the data ended inside the code
static inline int decode_symbol(Bits* b, const Huff* h) {
    const uint32_t v = b->peek16();
    int l = h->look_len[v >> 7], sym = 0;
    if (l) {
        sym = h->look_sym[v >> 7];
    } else {
        for (l = 10; l <= 16; ++l) {
            const int32_t code = (int32_t)(v >> (16 - l));
            if (code <= h->maxcode[l]) {
                sym = h->vals[h->valoff[l] + code];     // valoff[l] + code lies in [0, nvals): code >= the first code of length l
                break;
            }
        }
        if (l > 16) return -1;
    }
    if (l > b->nbits) return -2;
    b->nbits -= l;
    return sym;
}

static inline int32_t extend(int32_t v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

static inline bool entropy_decode(const uint8_t* d, int64_t n, const dgp_jpeg_info* info, int16_t* coef, uint16_t* qt, const char** why) {
    State s;
    if (!info || !coef || !qt) return err(why, "jpeg: null argument");
    if (!parse(d, n, &s, why)) return false;
    const dgp_jpeg_info& g = s.info;
    // the caller sized coef and qt from ITS info: it has to be this stream's
    if (info->width != g.width || info->height != g.height || info->ncomp != g.ncomp || info->sampling != g.sampling ||
        info->total_blocks != g.total_blocks || info->restart_interval != g.restart_interval || info->scan_offset != g.scan_offset)
        return err(why, "jpeg: the info does not belong to this stream");
    for (int c = 0; c < g.ncomp; ++c) memcpy(qt + 64 * c, s.qt[s.tq[c]], 64 * sizeof(uint16_t));
    const int hs = g.blocks_x[0] / g.mcus_x, vs = g.blocks_y[0] / g.mcus_y;
    int64_t comp_off[3] = {0, g.blocks[0], (int64_t)g.blocks[0] + g.blocks[1]};
    Bits b{d, g.scan_offset, n, 0, 0};
    int32_t pred[3] = {0, 0, 0};
    int64_t mcu = 0;
    for (int my = 0; my < g.mcus_y; ++my)
        for (int mx = 0; mx < g.mcus_x; ++mx, ++mcu) {
            if (g.restart_interval && mcu && mcu % g.restart_interval == 0) {
                // B.2.1, F.2.2.4: the rest of the byte is padding, then RSTm with m counting modulo 8
                if (b.nbits >= 8) return err(why, "jpeg: data where a restart marker was expected");
                b.nbits = 0;
                b.acc = 0;
                int64_t p = b.pos;
                if (p + 1 >= n || d[p] != 0xFF) return err(why, "jpeg: wrong restart marker");
                while (p + 1 < n && d[p + 1] == 0xFF) ++p;
                if (p + 1 >= n || d[p + 1] != 0xD0 + (int)((mcu / g.restart_interval - 1) & 7)) return err(why, "jpeg: wrong restart marker");
                b.pos = p + 2;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < g.ncomp; ++c) {
                const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
                const Huff* const hdc = &s.dc[s.td[c]];
                const Huff* const hac = &s.ac[s.ta[c]];
                const uint16_t* const q = s.qt[s.tq[c]];
                for (int by = 0; by < cv; ++by)
                    for (int bx = 0; bx < ch; ++bx) {
                        const int64_t blk = comp_off[c] + (int64_t)(my * cv + by) * g.blocks_x[c] + (mx * ch + bx);      // < total_blocks by construction
                        int16_t* const out = coef + blk * 64;
                        memset(out, 0, 64 * sizeof(int16_t));
                        int sym = decode_symbol(&b, hdc);
                        if (sym < 0) return err(why, sym == -1 ? "jpeg: a Huffman code runs past 16 bits" : "jpeg: the entropy-coded data ends early");
                        if (sym > 11) return err(why, "jpeg: DC category above 11");
                        int32_t v = 0;
                        if (sym) {
                            if (!b.take(sym, &v)) return err(why, "jpeg: the entropy-coded data ends early");
                            v = extend(v, sym);
                        }
                        pred[c] += v;
                        if (pred[c] > 32767 || pred[c] < -32767 || pred[c] * (int32_t)q[0] > 32767 || pred[c] * (int32_t)q[0] < -32767)
                            return err(why, "jpeg: |coefficient x table entry| above 32767");
                        out[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            sym = decode_symbol(&b, hac);
                            if (sym < 0) return err(why, sym == -1 ? "jpeg: a Huffman code runs past 16 bits" : "jpeg: the entropy-coded data ends early");
                            const int r = sym >> 4, sz = sym & 15;
                            if (sz == 0) {
                                if (r != 15) break;              // EOB
                                k += 16;                         // ZRL
                                continue;
                            }
                            k += r;
                            if (k > 63) return err(why, "jpeg: coefficient index past 63");
                            if (!b.take(sz, &v)) return err(why, "jpeg: the entropy-coded data ends early");
                            v = extend(v, sz);
                            const int nat = kZigzag[k];
                            if (v * (int32_t)q[nat] > 32767 || v * (int32_t)q[nat] < -32767) return err(why, "jpeg: |coefficient x table entry| above 32767");
                            out[nat] = (int16_t)v;
                            ++k;
                        }
                    }
            }
        }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the encoder's host half
// The mirror image: quantised coefficients (dgp_jpeg_forward_u8's, in the layout entropy_decode writes) -> the complete stream Pillow
// (libjpeg-turbo, default settings) writes for them: JFIF 1.01 header, the two tables, SOF0, the four Annex K.3 Huffman tables, one
// interleaved scan without restart markers (F.1.2).  The same rules: no globals, no allocation, every write checked against `cap`.

// Annex K.1 / K.2, natural order
static const uint8_t kStdLumQuant[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                         69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                         81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kStdChrQuant[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

constexpr int64_t kEncHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14;      // SOI .. SOS
// a block's worst case: a DC code of 11 bits + 11 value bits, 63 AC codes of 16 bits + 10 value bits = 1660 bits, every byte stuffed
constexpr int64_t kEncBlockBytes = 2 * ((22 + 63 * 26 + 7) / 8);

// libjpeg's jpeg_set_quality with force_baseline: qt[0] luminance, qt[1] chrominance, natural order
static inline bool quality_tables(int32_t quality, uint16_t* qt) {
    if (!qt || quality < 1 || quality > 100) return false;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = ((t ? kStdChrQuant[k] : kStdLumQuant[k]) * scale + 50) / 100;
            qt[t * 64 + k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return true;
}

// 0 for a geometry the encoder refuses (grey included)
static inline int64_t encode_bound(int32_t H, int32_t W, int32_t sampling) {
    dgp_jpeg_info g;
    if (sampling == DGP_JPEG_GRAY || !geometry(W, H, sampling, &g)) return 0;
    return kEncHeaderBytes + (int64_t)g.total_blocks * kEncBlockBytes + 2 + 2;          // + the padded last byte (stuffed if FF) + EOI
}

struct EncHuff {
    uint16_t code[256];
    uint8_t len[256];           // 0: the table has no code for the symbol
};

static inline void build_enc_huff(EncHuff* h, const uint8_t* bits, const uint8_t* vals) {
    memset(h->len, 0, sizeof(h->len));
    memset(h->code, 0, sizeof(h->code));
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            h->code[vals[k]] = (uint16_t)code;
            h->len[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

struct Out {
    uint8_t* d;
    int64_t pos, cap;
    uint64_t acc;
    int nbits;
    bool full;

    inline void byte(uint8_t b) {
        if (pos < cap) d[pos++] = b;
        else full = true;
    }
    inline void bytes(const uint8_t* s, int n) {
        for (int i = 0; i < n; ++i) byte(s[i]);
    }
    inline void u16(int v) {
        byte((uint8_t)(v >> 8));
        byte((uint8_t)(v & 255));
    }
    // `size` (1..32) bits of entropy-coded data, most significant first; a byte FF is followed by a stuffed 00 (B.1.1.5)
    inline void put(uint32_t code, int size) {
        acc = (acc << size) | code;      // at most 7 bits were left: 39 of the 64 in use
        nbits += size;
        while (nbits >= 8) {
            const uint8_t b = (uint8_t)(acc >> (nbits - 8));
            byte(b);
            if (b == 0xFF) byte(0);
            nbits -= 8;
        }
    }
};

static inline int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

static inline void put_dht(Out* o, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
    o->byte(0xFF);
    o->byte(0xC4);
    o->u16(19 + nvals);
    o->byte((uint8_t)tc_th);
    o->bytes(bits, 16);
    o->bytes(vals, nvals);
}

// coef: int16 [total_blocks][64] as entropy_decode writes it; qt: uint16 [2][64] natural order, entries 1..255.  *n = bytes written.
static inline bool entropy_encode(const int16_t* coef, int32_t H, int32_t W, int32_t sampling, const uint16_t* qt, uint8_t* out, int64_t cap,
                                  int64_t* n, const char** why) {
    if (!coef || !qt || !out || !n || cap < 0) return err(why, "jpeg: null argument");
    *n = 0;
    dgp_jpeg_info g;
    if (sampling == DGP_JPEG_GRAY) return err(why, "jpeg: the encoder writes 3-component streams only (sampling DGP_JPEG_444, _422 or _420)");
    if (!geometry(W, H, sampling, &g)) return err(why, "jpeg: H, W must be in 1..65535 and sampling one of DGP_JPEG_444, _422, _420");
    for (int k = 0; k < 128; ++k)
        if (qt[k] < 1 || qt[k] > 255) return err(why, "jpeg: a quantisation table entry outside 1..255 (baseline tables are 8-bit)");
    Out o{out, 0, cap, 0, 0, false};
    static const uint8_t kApp0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    o.bytes(kApp0, 20);
    for (int t = 0; t < 2; ++t) {
        o.byte(0xFF);
        o.byte(0xDB);
        o.u16(67);
        o.byte((uint8_t)t);
        for (int k = 0; k < 64; ++k) o.byte((uint8_t)qt[t * 64 + kZigzag[k]]);
    }
    const int hs = g.blocks_x[0] / g.mcus_x, vs = g.blocks_y[0] / g.mcus_y;
    o.byte(0xFF);
    o.byte(0xC0);
    o.u16(17);
    o.byte(8);
    o.u16(H);
    o.u16(W);
    o.byte(3);
    for (int c = 0; c < 3; ++c) {
        o.byte((uint8_t)(c + 1));
        o.byte((uint8_t)(c == 0 ? (hs << 4) | vs : 0x11));
        o.byte((uint8_t)(c ? 1 : 0));
    }
    put_dht(&o, 0x00, kStdDcLumBits, kStdDcVals, 12);
    put_dht(&o, 0x10, kStdAcLumBits, kStdAcLumVals, 162);
    put_dht(&o, 0x01, kStdDcChrBits, kStdDcVals, 12);
    put_dht(&o, 0x11, kStdAcChrBits, kStdAcChrVals, 162);
    static const uint8_t kSos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    o.bytes(kSos, 14);
    if (o.full) return err(why, "jpeg: the output buffer is smaller than the stream (dgp_jpeg_encode_bound gives a size that always fits)");

    EncHuff dc[2], ac[2];
    build_enc_huff(&dc[0], kStdDcLumBits, kStdDcVals);
    build_enc_huff(&dc[1], kStdDcChrBits, kStdDcVals);
    build_enc_huff(&ac[0], kStdAcLumBits, kStdAcLumVals);
    build_enc_huff(&ac[1], kStdAcChrBits, kStdAcChrVals);
    const int64_t comp_off[3] = {0, g.blocks[0], (int64_t)g.blocks[0] + g.blocks[1]};
    int32_t pred[3] = {0, 0, 0};
    for (int my = 0; my < g.mcus_y; ++my)
        for (int mx = 0; mx < g.mcus_x; ++mx) {
            for (int c = 0; c < 3; ++c) {
                const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
                const EncHuff* const hdc = &dc[c ? 1 : 0];
                const EncHuff* const hac = &ac[c ? 1 : 0];
                for (int by = 0; by < cv; ++by)
                    for (int bx = 0; bx < ch; ++bx) {
                        const int16_t* const blk = coef + (comp_off[c] + (int64_t)(my * cv + by) * g.blocks_x[c] + (mx * ch + bx)) * 64;
                        // F.1.2.1: the DC difference, category = bit length of its magnitude, then the low bits of v (v - 1 when negative)
                        int32_t v = (int32_t)blk[0] - pred[c];
                        pred[c] = blk[0];
                        int s = bit_length((uint32_t)(v < 0 ? -v : v));
                        if (s > 11) return err(why, "jpeg: a DC difference outside what category 11 can code (|d| > 2047)");
                        o.put(hdc->code[s], hdc->len[s]);
                        if (s) o.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s);
                        // F.1.2.2: run lengths of zeros in zigzag order, ZRL for runs past 15, EOB when the block ends in zeros
                        int run = 0;
                        for (int k = 1; k < 64; ++k) {
                            v = blk[kZigzag[k]];
                            if (v == 0) {
                                ++run;
                                continue;
                            }
                            for (; run > 15; run -= 16) o.put(hac->code[0xF0], hac->len[0xF0]);
                            s = bit_length((uint32_t)(v < 0 ? -v : v));
                            if (s > 10) return err(why, "jpeg: an AC coefficient outside what category 10 can code (|c| > 1023)");
                            const int sym = (run << 4) | s;
                            o.put(((uint32_t)hac->code[sym] << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), hac->len[sym] + s);
                            run = 0;
                        }
                        if (run) o.put(hac->code[0], hac->len[0]);
                    }
            }
            if (o.full) return err(why, "jpeg: the output buffer is smaller than the stream (dgp_jpeg_encode_bound gives a size that always fits)");
        }
    if (o.nbits) o.put((1u << (8 - o.nbits)) - 1u, 8 - o.nbits);      // the last byte is padded with 1-bits
    o.byte(0xFF);
    o.byte(0xD9);
    if (o.full) return err(why, "jpeg: the output buffer is smaller than the stream (dgp_jpeg_encode_bound gives a size that always fits)");
    *n = o.pos;
    return true;
}

}  // namespace dgp_jpeg

#endif /* DGP_JPEG_HOST_H */
