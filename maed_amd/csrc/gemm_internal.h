// Internal interface between the GEMM translation units (and block.hip's runtime set-up): what the dispatchers of gemm.hip / gemm_tn.hip call in the files that
// hold the kernels.  Definers and callers both include it.  Not part of the C-ABI.
#pragma once
#include "common.cuh"
#include "gemm_epilogue.cuh"

// csrc/gemm256.hip: 256x256 tiles with the counted-vmcnt LDS-DMA pipeline; false for epilogues the kernel does not carry (fp32 atomics: split-K)
bool maed_gemm_nt_256_launch(int epilogue, const void* A, int64_t lda, const void* B, int64_t ldb, int64_t M, int64_t N, int64_t K, const EpiArgs& e,
                             hipStream_t s);

// csrc/gemm_sk.hip: persistent K-stream kernel (256x256 tiles, one workgroup per CU, stream-K cuts) and the slabs of its hand-offs
bool maed_gemm_nt_sk_shape_ok(int64_t M, int64_t N, int64_t K);
bool maed_gemm_nt_sk_launch(int epilogue, const void* A, int64_t lda, const void* B, int64_t ldb, int64_t M, int64_t N, int64_t K, const EpiArgs& e,
                            int mode, int grid_opt, hipStream_t s);
int maed_sk_init(void);               // called once from maed_init_runtime (block.hip); safe to call again
int maed_sk_cus(void);
float* maed_sk_slab_set(hipStream_t s, size_t* bytes, int* ncu);      // the slab set of `s` (one slab per workgroup, no flags); NULL: no allocation / more streams than sets

// csrc/gemm_tn_sk.hip: persistent K-stream weight gradient
bool maed_gemm_tn_sk_ok(int64_t M, int N, int K, int64_t ldy, int64_t ldx, int64_t ldw, const void* Y, const void* X, const void* dW);
int maed_gemm_tn_sk_launch(const void* Y, int64_t ldy, const void* X, int64_t ldx, int64_t M, int N, int K, float* dW, int64_t ldw, float* dbias, int grid_opt,
                           hipStream_t s);

// csrc/gemm_tn2.hip: weight gradient on LDS-DMA copies and transposing reads
bool maed_gemm_tn_dma_ok(int64_t M, int N, int K, int64_t ldy, int64_t ldx);
int maed_gemm_tn_dma_launch(const void* Y, int64_t ldy, const void* X, int64_t ldx, int64_t M, int N, int K, float* dW, int64_t ldw, float* dbias, int which,
                            hipStream_t stream);
