// Packed-document (cu_seqlens) flash attention: the varlen kernels and
// launchers of flash_attn.hip, compiled as a module of their own so that
// the dense kernels' code objects are not perturbed (see the note above
// flash_varlen_fwd_kernel in flash_attn.hip).
#define GALV_FLASH_VARLEN_TU
#include "flash_attn.hip"
