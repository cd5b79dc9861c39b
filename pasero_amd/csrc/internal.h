// What crosses files inside libpasero_hip.so without being part of the C ABI: the error hook and the launchers one
// translation unit defines for another.  Each is declared HERE and nowhere else; the file that defines one and the files
// that call it all see this header (the .hip files through common.h), so a definition that drifts from its declaration is
// a "conflicting types" error.  The same holds for the public entry points through include/pasero_hip.h, pulled in below.
// The functions stay extern "C" — exports.map (tools/gen_exports.py) keeps everything the public header does not declare
// local to the library.  No HIP headers: layer.cpp and capi.cpp are host-only.
// (The long-sequence attention launchers take a C++ reference and live in attention_common.h.)
#pragma once
#include "../../include/pasero_hip.h"
#include "gemm_epi.h"

extern "C" {

void pk_set_error(const char* fmt, ...);  // capi.cpp: the message pk_last_error() returns (thread-local)

// ---- the kernels behind pk_gemm / pk_gemm_wgrad_group / pk_gemm_ln_fwd / pk_gemm_relu_bits (dispatch: gemm.hip) ----
// gemm256.hip
int pk_gemm256_launch(const void* A, const void* B, void* C, float* ws, float* asum_ws, void* asum_out, long long M,
                      long long N, long long K, long long lda, long long ldb, int a_col, int b_col, int kchunk, int splitk,
                      EpiParams ep, int dtype, void* stream);
// gemm8p.hip
int pk_gemm8p_eligible(long long M, long long N, long long K, long long lda, long long ldb, int a_col, int b_col,
                       int want_asum);
int pk_gemm8p_is_pw(long long M, long long N, long long K, long long lda, long long ldb, int a_col, int b_col, int splitk,
                    int has_ws, int has_asum, const EpiParams* ep);
int pk_gemm8p_is_pt(long long M, long long N, long long K, long long lda, long long ldb, int a_col, int b_col, int splitk,
                    int has_ws, int has_asum, const EpiParams* ep);
int pk_gemm8p_launch(const void* A, const void* B, void* C, float* ws, float* asum_ws, void* asum_out, long long M,
                     long long N, long long K, long long lda, long long ldb, int a_col, int b_col, int kchunk, int splitk,
                     EpiParams ep, int dtype, void* stream);
int pk_gemm8p_group_eligible(const PkWgradProblem* q);
int pk_gemm8p_group_plan(const PkWgradProblem* p, int n, size_t* ws_bytes, int* workgroups, int* slabs);
int pk_gemm8p_group_map(const PkWgradProblem* p, int n, int* out, int cap);
int pk_gemm8p_group_launch(const PkWgradProblem* p, int n, int dtype, float* workspace, void* stream);
int pk_gemm8p_group_reduce(const PkWgradProblem* p, int n, int dtype, float* workspace, void* stream);
// gemmpw.hip (called from gemm8p.hip)
int pk_gemmpw_eligible(long long M, long long N, long long K, long long lda, long long ldb, long long ldc, int b_col,
                       const EpiParams* ep);
int pk_gemmpw_launch(const void* A, const void* B, void* C, long long M, long long N, long long K, long long lda,
                     long long ldb, unsigned a_bytes, unsigned b_bytes, int b_col, EpiParams ep, int dtype, void* stream);
// gemmln.hip
int pk_gemmln_spec(int has_residual, float drop_p, long long K);
int pk_gemmln_launch(const void* A, const void* W, const void* bias, const void* residual, const void* gamma,
                     const void* beta, void* z_out, void* y_out, float* mean, float* rstd, long long M, long long N,
                     long long K, long long lda, long long ldb, long long ldr, float eps, float drop_p,
                     unsigned long long seed, unsigned long long offset, int dtype, void* stream);
// gemmbs.hip
int pk_gemmbs_eligible(const void* A, const void* B, const void* C, long long M, long long N, long long K, long long lda,
                       long long ldb, int a_col, int b_col, const EpiParams* ep);
int pk_gemmbs_launch(const void* A, const void* B, void* C, long long M, long long N, long long K, long long lda,
                     long long ldb, int b_col, EpiParams ep, int dtype, void* stream, unsigned char* bits, long long ldbits);
int pk_gemmbs_use(int on);
// gemm_skinny.hip
int pk_gemm_skinny_launch(const void* A, const void* B, void* C, long long M, long long N, long long K, long long lda,
                          long long ldb, EpiParams ep, int dtype, void* stream);

// ---- adapter.hip: pk_adapter_rows as the decoding step runs it (decode.hip; the route pk_adapter_step_fused selects) ----
size_t pk_adapter_rows_step_scratch(long long rows, int d, int p, int dtype);
int pk_adapter_rows_step(const void* x, void* y, const void* ln_g, const void* ln_b, const void* down_w, const void* down_b,
                         const void* up_w, const void* up_b, long long rows, int d, int p, int act, float scaling, float eps,
                         int dtype, void* scratch, size_t scratch_bytes, void* stream);

}  // extern "C"
