// The three-plane bf16 image of a packed table (sga_loss_split3_tables; sweep3.hip describes the arithmetic and the layout) as the kernels
// that read it see it: sweep3.hip (the anchors x negatives sweeps, the stash products) and anchor3.hip (the anchors x anchors pass).
#pragma once
#include "loss_math.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int S3_DP = 104;
constexpr int S3_PLANE = 3 * 2 * 1024;           // 6144 B
constexpr int S3_TAIL = 3 * S3_PLANE;            // byte offset of the tail image in a block
constexpr int S3_BLOCK = S3_TAIL + 2048;         // 20480 B
constexpr int S3_NCH = S3_BLOCK / 1024;          // 20 DMA chunks
constexpr int S3_ROWSLOTS = 3 * 12 + 4;          // 16-byte slots that hold one row: 3 planes x (3 K steps x 4 k groups) + the tail image's 4 k groups

__device__ __forceinline__ f32x4 mfma_b(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__host__ __device__ constexpr int s3_slot(int g, int i) { return 16 * g + (i ^ (12 * (g & 1))); }

struct TLayout { int nbA, nb1, nb2; };
__host__ __device__ inline TLayout make_tlayout(int A, int J1, int J2) { return TLayout{(A + 31) / 32, (J1 + 31) / 32, (J2 + 31) / 32}; }

// The owner side's two K-tail operands from its row's tail slots th, tm, tl (columns 96 .. 103 of the h, m, l planes), for the lane's k group
// g4.  Against the image's k groups (h, h, m, l):  O0 = (h, m, h, h) -> h h + h m + m h + l h;  O1 = (l, 0, m, 0) -> h l + m m.  Columns
// 100, 101 swapped: the owner holds (1, b_i) against the other's (b_j, 1).
__device__ __forceinline__ void s3_own_tails(const u32x4 th, const u32x4 tm, const u32x4 tl, const int g4, u32x4 (&otl)[2]) {
    otl[0] = g4 == 1 ? tm : th;
    otl[1] = g4 == 0 ? tl : (g4 == 2 ? tm : u32x4{0, 0, 0, 0});
#pragma unroll
    for (int t = 0; t < 2; ++t) otl[t][2] = (otl[t][2] >> 16) | (otl[t][2] << 16);
}

}  // namespace
