// Device helpers shared by the attention kernels (attention.hip: base model, attention2.hip: two-stream model), gfx950.
//
// Swizzled LDS image: [rows][64] bf16, 128-B rows of eight 16-B chunks, chunk c of row r stored at c ^ (r & 7).  Read by rows
// with ds_read_b128 (row_frag) and by columns with ds_read_b64_tr_b16 (col_frag) -- both conflict-free on the same image.
#pragma once
#include "common.h"

// hand-placed MFMA -> VALU wait states where a branch follows an MFMA chain (tools/check_mfma_hazard.py is the build-time guard;
// -DATTN_NO_HAZARD_PAD builds the deliberately broken variant the guard must flag)
#ifdef ATTN_NO_HAZARD_PAD
#define HAZARD_PAD()
#else
#define HAZARD_PAD() asm volatile("s_nop 15\n\ts_nop 7" ::: "memory")
#endif
#define NT_MAX 13            // 13 * 16 = 208 >= 197 tokens
#define ROWS_PAD 224         // 14 * 16: k-steps pair two 16-row tiles
#define IMG_BYTES (ROWS_PAD * 128)
#define LOG2E 1.4426950408889634f
#define NEG_BIG (-1e30f)

__device__ __forceinline__ int img_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

__device__ __forceinline__ bf16x8 row_frag(const char* img, int row, int chunk) {
    return *(const bf16x8*)(img + img_off(row, chunk));
}

// operand element j of lane (g, i):  img[row = (j<4 ? r_lo : r_hi) + 4g + (j&3)][col0 + i]
__device__ __forceinline__ bf16x8 col_frag(const char* img, int r_lo, int r_hi, int col0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int chunk = (col0 >> 3) + (p >> 1), within = (p & 1) << 3;
    const int ra = r_lo + 4 * g + q, rb = r_hi + 4 * g + q;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, img + img_off(ra, chunk) + within));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, img + img_off(rb, chunk) + within));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// One 1-KiB LDS-DMA piece (global_load_lds, 16 B per lane, no VGPR round trip): source rows row0 + 8 rb .. row0 + 8 rb + 7 of a
// [rows][64] bf16 source land as image rows 8 rb .. 8 rb + 7 -- lane l writes LDS byte rb * 1024 + 16 l = img_off(8 rb + (l >> 3),
// chunk) for chunk = (l & 7) ^ (l >> 3), so the swizzle is applied on the SOURCE side.  Rows >= n_valid re-read row n_valid - 1 (the
// DMA cannot zero-fill): the user must mask padded rows arithmetically (the forward's -1e30 bias columns give p = 0 for padded
// keys, and 0 x finite = 0 in P.V), so they only need to be finite.  `img` and `rb` must be wave-uniform.
__device__ __forceinline__ void dma_rows8(char* img, int rb, const bf16* src, size_t stride, int row0, int n_valid, int lane) {
    const int row = row0 + 8 * rb + (lane >> 3);
    const int chunk = (lane & 7) ^ (lane >> 3);
    const int r = row < n_valid ? row : n_valid - 1;
    __builtin_amdgcn_global_load_lds(GLB_PTR(void, src + (size_t)r * stride + chunk * 8), LDS_PTR(void, img + rb * 1024), 16, 0, 0);
}

// After an explicit `s_waitcnt vmcnt(0)`: tell the compiler's wait-count tracking that a prefetched register HAS landed (it inserts
// its own, by then free, wait in front of this use).  Without it the first real use -- on the far side of a loop back-edge and
// behind newly issued stores, which the in-order vmcnt cannot skip -- waits for those as well.
__device__ __forceinline__ void landed(bf16x8& v) { asm volatile("" : "+v"(v)); }

__device__ __forceinline__ bf16x8 pack8(const float* a, const float* b) {
    bf16x8 v = {f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(b[0]), f2bf(b[1]), f2bf(b[2]), f2bf(b[3])};
    return v;
}

// Dropout: one 32-bit hash per (query row, key pair); each key takes a 16-bit half and is kept when
// half >= round(p * 65536).  pair index = (bh*N + q) * (NP/2) + (key >> 1).  Mirrored by
// oracle/vit_oracle.py::attn_keep_mask.
__device__ __forceinline__ uint32_t pair_hash(uint32_t key32, uint32_t pidx) {
    uint32_t x = (pidx ^ key32) * 0x9E3779B1u;
    x ^= x >> 15; x *= 0x85EBCA77u; x ^= x >> 13;
    return x;
}
// keep flags of the 4 consecutive keys kbase..kbase+3 (kbase % 4 == 0) of one query row
__device__ __forceinline__ void keep4(uint32_t key32, uint32_t rowpair, int kbase, uint32_t thr16, bool (&k)[4]) {
    const uint32_t h0 = pair_hash(key32, rowpair + (kbase >> 1)), h1 = pair_hash(key32, rowpair + (kbase >> 1) + 1);
    k[0] = (h0 & 0xFFFFu) >= thr16; k[1] = (h0 >> 16) >= thr16;
    k[2] = (h1 & 0xFFFFu) >= thr16; k[3] = (h1 >> 16) >= thr16;
}
__device__ __forceinline__ bool keep1(uint32_t key32, uint32_t rowpair, int key, uint32_t thr16) {
    const uint32_t h = pair_hash(key32, rowpair + (key >> 1));
    return ((key & 1) ? (h >> 16) : (h & 0xFFFFu)) >= thr16;
}

__device__ __forceinline__ float group_sum4(float v) {   // sum over the 4 lane groups (lanes l, l^16, l^32, l^48)
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float group_max4(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}
