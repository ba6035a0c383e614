// Packed-document flash attention on the packed-QKV buffer: the
// flash_packed_varlen_* kernels and launchers of flash_attn.hip, compiled
// as a module of their own so that the other flash kernels' code objects
// are not perturbed (see the notes above flash_varlen_fwd_kernel and
// flash_packed_varlen_fwd_kernel in flash_attn.hip).
#define GALV_FLASH_PACKED_VARLEN_TU
#include "flash_attn.hip"
