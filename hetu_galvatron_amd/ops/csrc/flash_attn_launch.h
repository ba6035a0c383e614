// Host launchers of the flash-attention modules, declared once: each module
// includes this next to its definitions and bindings.hip next to its calls,
// so a definition and a call cannot drift apart.  d is the head dimension
// (64 | 128); layouts are in flash_attn_body.h and the modules.
#pragma once

#include <hip/hip_runtime.h>

// flash_attn.hip (dense)
void flash_fwd_launch(const __bf16* q, const __bf16* k, const __bf16* v,
                      __bf16* o, float* lse, int b, int sq, int skv, int hq,
                      int hkv, int d, float scale, bool causal,
                      hipStream_t st, const __bf16* bias = nullptr,
                      bool sbhd = false, int window = 0);
void attn_di_launch(const __bf16* dout, const __bf16* o, float* di, int b,
                    int sq, int hq, int d, hipStream_t st, bool sbhd = false);
void flash_bwd_launch(const __bf16* dout, const __bf16* q, const __bf16* k,
                      const __bf16* v, const float* lse, const float* di,
                      __bf16* dq, __bf16* dk_exp, __bf16* dv_exp, int b,
                      int sq, int skv, int hq, int hkv, int d, float scale,
                      bool causal, hipStream_t st,
                      const __bf16* bias = nullptr, float* dbias = nullptr,
                      bool sbhd = false, int window = 0);
void mfma_probe_launch(const __bf16* A, const __bf16* B, float* Dst, bool alt,
                       hipStream_t st);

// flash_attn_varlen.hip
void flash_varlen_fwd_launch(const __bf16* q, const __bf16* k,
                             const __bf16* v, __bf16* o, float* lse,
                             const int* cu, int nseg, int max_seqlen, int b,
                             int s, int hq, int hkv, int d, float scale,
                             bool causal, bool sbhd, hipStream_t st);
void flash_varlen_bwd_launch(const __bf16* dout, const __bf16* q,
                             const __bf16* k, const __bf16* v,
                             const float* lse, const float* di, __bf16* dq,
                             __bf16* dk_exp, __bf16* dv_exp, const int* cu,
                             int nseg, int max_seqlen, int b, int s, int hq,
                             int hkv, int d, float scale, bool causal,
                             bool sbhd, hipStream_t st);

// flash_attn_qkv.hip
void flash_packed_fwd_launch(const __bf16* qkv, __bf16* o, float* lse, int b,
                             int s, int G, int qpg, int d, float scale,
                             bool causal, hipStream_t st);
void flash_packed_bwd_launch(const __bf16* dout, const __bf16* qkv,
                             const float* lse, const float* di, __bf16* dqkv,
                             __bf16* dk_exp, __bf16* dv_exp, int b, int s,
                             int G, int qpg, int d, float scale, bool causal,
                             hipStream_t st);

// flash_attn_qkv_varlen.hip
void flash_packed_varlen_fwd_launch(const __bf16* qkv, __bf16* o, float* lse,
                                    const int* cu, int nseg, int max_seqlen,
                                    int b, int s, int G, int qpg, int d,
                                    float scale, bool causal,
                                    hipStream_t st);
void flash_packed_varlen_bwd_launch(const __bf16* dout, const __bf16* qkv,
                                    const float* lse, const float* di,
                                    __bf16* dqkv, __bf16* dk_exp,
                                    __bf16* dv_exp, const int* cu, int nseg,
                                    int max_seqlen, int b, int s, int G,
                                    int qpg, int d, float scale, bool causal,
                                    hipStream_t st);
