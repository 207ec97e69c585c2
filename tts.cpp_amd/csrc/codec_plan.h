// codec_plan.h — which packed image a codec convolution weight gets: its kind, its tile facts and its size, from the layer's role and
// dims and the layout knobs.  Decided once, when the image is made (shim_codec.hip: ensure_packed, ensure_packed_snac, Kokoro's lazy
// pack); the launchers dispatch on what the image records.  No HIP in here: tests/codec_plan_main.cpp builds it with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// input channels per LDS chunk of the fp32 k=1 kernels: 16 keeps the footprint at 40-45 KB (3-4 workgroups per CU);
// with 32 the 96- and 64-channel tiles needed 80-90 KB = ONE workgroup per CU, and a k=1 conv has only C/32 chunks to
// pipeline over, so its residual loads and stores ran with nothing to overlap (0.88 TB/s)
#define CI32_K1 16
// k=7: 4 channels per chunk (40 KB, 4 workgroups per CU) measured 3.7 % faster than 8 (75 KB, 2 per CU)
#ifndef CI32_T
#define CI32_T 8
#endif
#ifndef CI32_K7
#define CI32_K7 4
#endif
#define CI16_K7 16
#define CI16_K1 32
#define CI16_T  16

enum CodecKind : uint8_t {
    IMG_NONE = 0,        // no image: the layer runs on a kernel that reads the GGUF layout
    IMG_F32_TILE,        // conv1d_mfma_kernel / convt1d_mfma_kernel: [co tile][chunk][tap][ci_t][co_t] fp32
    IMG_F32_DIRECT,      // conv1x1_direct_kernel: [cin][cout] fp32
    IMG_F16_TILE,        // conv1d_mfma16_kernel / convt1d_mfma16_kernel: the tile layout in fp16
    IMG_B3,              // conv1d_mfma_b3_kernel: k-tap planes in tap pairs, fp32 activations
    IMG_PLANES,          // conv_b3p_kernel: planes in stage order, activations arrive as planes
    IMG_UNIT_PAIR,       // resunit_b3_kernel: a residual unit's stage stream, tap pairs (three bf16 planes only)
    IMG_UNIT_TAP,        // resunit_t7_kernel: ... one tap per k-step
    IMG_CONVT_PLANES,    // convt_b3_kernel: transposed conv on planes
};
enum CodecRole : uint8_t { ROLE_INIT, ROLE_UNIT7, ROLE_UNIT1, ROLE_CONVT, ROLE_SNAC_POINTWISE, ROLE_SNAC_CONVT, ROLE_KOKORO_SAME, ROLE_KOKORO_CONVT };

// what decides a layout: tts_hip_tune's layout keys plus two facts of the context (VALU flag, F16 codec tensors).  A change of any
// field after images exist drops them (drop_codec_images)
struct CodecKnobs {
    int valu = 0, f16 = 0;
    int b3 = 2, fuse = 1, planes = 1, split = 1, f16_planes = 1, tap7 = 1, convt_b3 = 1, conv1_direct = 1;
    int kk_split = 1, kk_b3 = 1, kk_mfma = 1;
    bool operator==(const CodecKnobs &o) const { return memcmp(this, &o, sizeof o) == 0; }   // ints only: no padding
};

struct CodecImage {
    void *w = nullptr;       // device image (NULL in a plan)
    uint8_t kind = IMG_NONE;
    uint8_t scheme = 0;      // operand split it was packed for: 0 = three bf16 planes, 1 = fp16 hi + lo, 2 = one fp16 plane (F16 tensors)
    uint8_t transposed = 0;
    int kt = 0;              // taps in the image (transposed: 2 x stride)
    int co_t = 0;            // output channels per tile
    int ci_t = 0;            // tile kinds: input channels per chunk
    int ns = 0;              // IMG_PLANES: k-steps per chunk (7: one tap per step, 4: tap pairs, 1: k = 1)
    size_t elems = 0;
};

static inline int codec_planes(int scheme) { return scheme == 0 ? 3 : scheme == 1 ? 2 : 1; }
// output-channel tile of the tile kernels (0: no tile form)
static inline int conv_co_tile(int cout, int K) {
    if (K != 7 && K != 1) return 0;
    if (cout % 128 == 0) return 128;
    if (cout % 96 == 0 && cout % 64 != 0) return 96;
    return cout % 64 == 0 ? 64 : 0;
}
static inline int convt_co_tile(int cout, int s) {
    if ((s == 8 || s == 4) && cout % 64 == 0) return 64;
    if (s == 2 && cout % 96 == 0) return 96;
    return s == 2 && cout % 64 == 0 ? 64 : 0;
}
// residual units of 96 / 192 channels as one launch: k-steps per stage of the k = 7 / k = 1 part
static inline bool resunit_shape(int C, int *KS, int *KS2) {
    if (C == 96) { *KS = 4; *KS2 = 3; return true; }
    if (C == 192) { *KS = 2; *KS2 = 4; return true; }
    return false;
}
// transposed convs on planes (convt_b3_kernel): 32 MI output channels per workgroup
static inline int convt_b3_tile(int cout, int cin, int s) {
    if (cin % 16) return 0;
    if (s == 8 && cout % 32 == 0) return 32;
    if (s == 4 && cout % 64 == 0) return 64;
    if (s == 2 && cout % 96 == 0) return 96;
    return 0;
}
static inline bool convt_b3_fits(int cout, int cin, int s) {   // the kernel's LDS request (weight stages + input planes + alpha) inside a CU's 160 KB (three planes: the largest scheme)
    const int t = convt_b3_tile(cout, cin, s);
    return t && (size_t) 6 * (2 * s * 2 * t * 8) * 2 + 6 * 2 * 257 * 8 * 2 + (size_t) cin * 8 <= 160 * 1024;
}
// wide classes on split planes (conv_b3p_kernel)
static inline bool planes_class(const CodecKnobs &k, int ch) {
    int ks = 0, ks2 = 0;
    return k.planes && k.b3 && (!k.f16 || k.f16_planes) && ch % 128 == 0 && !(k.fuse && resunit_shape(ch, &ks, &ks2));
}
// operand split of the plane kernels / of conv1d_mfma_b3_kernel (never the one-plane scheme: F16 tensors do not reach it)
static inline int dac_scheme(const CodecKnobs &k) { return k.f16 ? 2 : (k.split ? 1 : 0); }

static inline CodecImage plan_tile(uint8_t kind, int cout, int cin, int kt, int co_t, int ci_t, bool transposed) {
    CodecImage p;
    if (!co_t) return p;
    p.kind = kind; p.kt = kt; p.co_t = co_t; p.ci_t = ci_t; p.transposed = transposed;
    p.elems = (size_t) ((cout + co_t - 1) / co_t) * ((cin + ci_t - 1) / ci_t) * kt * ci_t * co_t;
    return p;
}
static inline CodecImage plan_b3(int cout, int cin, int kt, int co_t, int scheme) {   // 8 input channels per chunk, tap pairs
    CodecImage p;
    p.kind = IMG_B3; p.scheme = (uint8_t) scheme; p.kt = kt; p.co_t = co_t; p.ci_t = 8;
    p.elems = (size_t) ((cout + co_t - 1) / co_t) * ((cin + 7) / 8) * codec_planes(scheme) * (2 * ((kt + 1) / 2)) * co_t * 8;
    return p;
}
// k = 7 in 64-channel tiles (four k-steps of tap pairs per 8-channel chunk, or seven of one tap per 16-channel chunk), k = 1 in 128- /
// 256-channel tiles (one k-step = 16 channels per chunk)
static inline CodecImage plan_planes(const CodecKnobs &k, int cout, int cin, int kt) {
    const bool tapk = kt == 7 && k.tap7 && cin % 16 == 0;
    CodecImage p;
    p.kind = IMG_PLANES; p.scheme = (uint8_t) dac_scheme(k); p.kt = kt;
    p.co_t = kt == 7 ? 64 : (cout % 256 == 0 ? 256 : 128);
    p.ns = kt == 7 ? (tapk ? 7 : 4) : 1;
    p.ci_t = kt == 7 && !tapk ? 8 : 16;
    p.elems = (size_t) (cout / p.co_t) * (cin / p.ci_t) * codec_planes(p.scheme) * p.ns * 2 * p.co_t * 8;
    return p;
}
static inline CodecImage plan_unit(const CodecKnobs &k, int C) {
    int KS = 0, KS2 = 0;
    CodecImage p;
    if (!resunit_shape(C, &KS, &KS2)) return p;
    p.kt = 7; p.co_t = C;
    if (k.tap7) {   // stages of {4, 3} / {2, 2, 2, 1} k-steps per 16-channel chunk
        const int MI = C / 32, SPC = MI == 3 ? 2 : 4, MAXCNT = MI == 3 ? 4 : 2;
        p.kind = IMG_UNIT_TAP; p.scheme = (uint8_t) dac_scheme(k); p.ci_t = 16;
        p.elems = (size_t) ((C / 16) * SPC + (C / 96) * ((C / 16) / KS2) + 1) * ((size_t) codec_planes(p.scheme) * MAXCNT * 2 * C * 8);
    } else {        // resunit_geom (dac_b3_kernels.h); + 1: the prefetch of the stage after the last one stays inside the buffer
        const int a = 3 * KS * 2 * C * 8, b = 3 * KS2 * 2 * 96 * 8;
        p.kind = IMG_UNIT_PAIR; p.scheme = 0; p.ci_t = 8;
        p.elems = (size_t) ((C / 8) * (4 / KS) + (C / 96) * ((C / 16) / KS2) + 1) * (size_t) (a > b ? a : b);
    }
    return p;
}
static inline CodecImage plan_convt_planes(const CodecKnobs &k, int cout, int cin, int s) {
    CodecImage p;
    p.kind = IMG_CONVT_PLANES; p.scheme = (uint8_t) dac_scheme(k); p.transposed = 1; p.kt = 2 * s; p.co_t = convt_b3_tile(cout, cin, s); p.ci_t = 16;
    p.elems = (size_t) (cout / p.co_t) * (cin / 16) * codec_planes(p.scheme) * 2 * s * 2 * p.co_t * 8;
    return p;
}

// The one decision.  Every weight gets the ONE image the kernel that will run it stages (the images are as large as the weights: a second
// format per tensor would be dead device memory in every context).  A fused unit is planned under its k = 7 weight; its k = 1 weight has none.
// F16 codec tensors (quantize --convert-dac-to-f16): on the same plane / fused-unit / transposed kernels as F32 tensors with one fp16 plane
// (f16p); layers those kernels do not cover, and every layer when a switch takes them away, keep the fp16 tile kernels.
// dil: ROLE_KOKORO_SAME only (conv1d_mfma_b3_kernel's LDS holds dilations up to 5).
static inline CodecImage codec_plan(CodecRole role, int cout, int cin, int K, int stride, const CodecKnobs &k, int dil = 1) {
    CodecImage none;
    if (k.valu) return none;
    const bool f16p = k.f16 && k.f16_planes && k.b3 && k.tap7, f16_tiles = k.f16 && !f16p;
    int ks = 0, ks2 = 0;
    switch (role) {
    case ROLE_INIT:
        if (f16_tiles) return plan_tile(IMG_F16_TILE, cout, cin, 7, conv_co_tile(cout, 7), CI16_K7, false);
        if (planes_class(k, cout) && cin % 8 == 0) return plan_planes(k, cout, cin, 7);
        if (f16p) return plan_tile(IMG_F16_TILE, cout, cin, 7, conv_co_tile(cout, 7), CI16_K7, false);
        if (k.b3 && cout % 64 == 0) return plan_b3(cout, cin, 7, 64, k.split ? 1 : 0);
        return plan_tile(IMG_F32_TILE, cout, cin, 7, conv_co_tile(cout, 7), CI32_K7, false);
    case ROLE_CONVT:
        if (f16_tiles) return plan_tile(IMG_F16_TILE, cout, cin, 2 * stride, convt_co_tile(cout, stride), CI16_T, true);
        if (k.convt_b3 && convt_b3_fits(cout, cin, stride)) return plan_convt_planes(k, cout, cin, stride);
        if (f16p) return plan_tile(IMG_F16_TILE, cout, cin, 2 * stride, convt_co_tile(cout, stride), CI16_T, true);
        return plan_tile(IMG_F32_TILE, cout, cin, 2 * stride, convt_co_tile(cout, stride), CI32_T, true);
    case ROLE_UNIT7:
    case ROLE_UNIT1: {
        const int kt = role == ROLE_UNIT7 ? 7 : 1;
        if (f16_tiles) return plan_tile(IMG_F16_TILE, cout, cin, kt, conv_co_tile(cout, kt), kt == 7 ? CI16_K7 : CI16_K1, false);
        if (planes_class(k, cout)) return plan_planes(k, cout, cin, kt);
        if (k.fuse && resunit_shape(cout, &ks, &ks2)) return kt == 7 ? plan_unit(k, cout) : none;   // one launch per unit (dilations 1 / 3 / 9 all qualify)
        if (f16p) return plan_tile(IMG_F16_TILE, cout, cin, kt, conv_co_tile(cout, kt), kt == 7 ? CI16_K7 : CI16_K1, false);
        if (kt == 7) {
            if (k.b3 && cout % 64 == 0) return plan_b3(cout, cin, 7, 64, k.split ? 1 : 0);
            if (k.b3 >= 2 && cout % 96 == 0) return plan_b3(cout, cin, 7, 96, k.split ? 1 : 0);
            return plan_tile(IMG_F32_TILE, cout, cin, 7, conv_co_tile(cout, 7), CI32_K7, false);
        }
        // the k = 1 conv of an unfused unit at <= 192 channels: [cin][cout] for conv1x1_direct_kernel (96-channel tiles; fp32 tensors only)
        if (k.conv1_direct && cout == cin && (cin == 96 || cin == 192)) return plan_tile(IMG_F32_DIRECT, cout, cin, 1, cout, CI32_K1, false);
        return plan_tile(IMG_F32_TILE, cout, cin, 1, conv_co_tile(cout, 1), CI32_K1, false);
    }
    case ROLE_SNAC_POINTWISE: return plan_tile(IMG_F32_TILE, cout, cin, 1, conv_co_tile(cout, 1), CI32_K1, false);
    case ROLE_SNAC_CONVT: return plan_tile(IMG_F32_TILE, cout, cin, 2 * stride, convt_co_tile(cout, stride), CI32_T, true);
    case ROLE_KOKORO_SAME:   // stride-1 "same" convolutions k = 1 / 3 / 5 / 7 / 11 of at least 16 channels
        if (!k.kk_mfma || cout < 16 || cin < 16) return none;
        // other widths (conv_post: 22 channels): 64-channel tiles, zero-padded weights, stores masked
        if (K == 1) return plan_tile(IMG_F32_TILE, cout, cin, 1, cout % 128 == 0 ? 128 : 64, 16, false);
        if (K != 3 && K != 5 && K != 7 && K != 11) return none;
        if (k.kk_b3 && dil <= 5) return plan_b3(cout, cin, K, 64, k.kk_split ? 1 : 0);
        return plan_tile(IMG_F32_TILE, cout, cin, K, cout % 128 == 0 ? 128 : 64, K == 3 ? 8 : 4, false);
    case ROLE_KOKORO_CONVT:  // the generator's ConvTranspose1d (stride 10 / 6, kernel = 2 x stride)
        if (!k.kk_mfma || K != 2 * stride || (stride != 10 && stride != 6) || cout % 64) return none;
        return plan_tile(IMG_F32_TILE, cout, cin, K, 64, CI32_T, true);
    }
    return none;
}
