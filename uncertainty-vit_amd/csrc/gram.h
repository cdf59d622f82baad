// X^T X over the rows of a batch, one 64 x 64 output tile per workgroup of 256 threads with a 4 x 4 micro-tile each: the reduction
// shared by the Kronecker factors of laplace.hip and the scatter matrix of maha.hip.
#pragma once

#define GRAM_T 64            // output tile edge
#define GRAM_K 16            // batch rows per LDS tile

// x(b, col) is the double element of batch row b in column col, 0.0 past the matrix and in a row that is left out.  Thread
// (ty, tx) = (tid / 16, tid % 16) gets acc[i][j] += sum_b x(b, i0 + 4 ty + i) x(b, j0 + 4 tx + j), one fma chain over b in ascending
// order, and, with ROWSUM, si[i] += sum_b x(b, i0 + 4 ty + i).  (i, j) and (j, i) are formed from the same products (a * b == b * a)
// in the same order: a caller that adds acc to a symmetric matrix by one expression keeps it symmetric bit for bit.
template <bool ROWSUM, class X>
__device__ __forceinline__ void gram_tile(X x, int B, int i0, int j0, double (&acc)[4][4], double (&si)[4]) {
    __shared__ __attribute__((aligned(16))) double Is[GRAM_K][GRAM_T + 2], Js[GRAM_K][GRAM_T + 2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int fr = tid >> 4, fc = (tid & 15) * 4;         // staging: batch row, first of four columns
    for (int b0 = 0; b0 < B; b0 += GRAM_K) {
        double vi[4], vj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            vi[q] = x(b0 + fr, i0 + fc + q);
            vj[q] = x(b0 + fr, j0 + fc + q);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) { Is[fr][fc + q] = vi[q]; Js[fr][fc + q] = vj[q]; }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < GRAM_K; ++b) {                // rows past B hold zeros: fma(0, 0, acc) = acc
            const double2 i01 = *(const double2*)&Is[b][ty * 4], i23 = *(const double2*)&Is[b][ty * 4 + 2];
            const double2 j01 = *(const double2*)&Js[b][tx * 4], j23 = *(const double2*)&Js[b][tx * 4 + 2];
            const double ii[4] = {i01.x, i01.y, i23.x, i23.y}, jj[4] = {j01.x, j01.y, j23.x, j23.y};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (ROWSUM) si[i] += ii[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(ii[i], jj[j], acc[i][j]);
            }
        }
    }
}
