/*
 * wo_denoise.h -- internal C ABI of the a-trous denoiser (renderer_ext.h wo_denoise_*):
 * between the host unit (denoise.c: argument checks, defaults, scratch size, the host
 * filter), the renderer (renderer.c: the public device entry points) and the HIP unit
 * (denoise_kernels.hip: the kernels and their launches).  Not installed.
 */
#ifndef WOLOLO_WO_DENOISE_H
#define WOLOLO_WO_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#include "wololo/renderer/renderer_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* denoise.c: the checks of wo_denoise_device / wo_denoise_host in the header's order; `what`
 * prefixes the message.  check_params: NULL .. a bad k_* (1-5); check_extent: width, height (6);
 * check_planes: required planes, alignment, overlap, short scratch (7-10), `scratch` and
 * `scratch_bytes` only when `device` (the host form has none).  0, or -1 (wo_set_error). */
int wo_denoise_check_params(char const* what, Wo_DenoiseParams const* dp);
int wo_denoise_check_extent(char const* what, uint32_t width, uint32_t height);
int wo_denoise_check_planes(char const* what, Wo_DenoiseParams const* dp, uint32_t width, uint32_t height,
                            void const* color, void const* albedo, void const* normal, void const* ids, void const* out,
                            void const* scratch, size_t scratch_bytes, int device);

/* denoise_kernels.hip: the launches of one checked call on the current device, async on `stream`. */
int wo_dev_denoise(Wo_DenoiseParams const* dp, uint32_t width, uint32_t height, void const* d_color,
                   void const* d_albedo, void const* d_normal, void const* d_ids, void* d_out, void* d_scratch,
                   void* stream, char* err, size_t errlen);
/* Device buffers of a synchronous whole-frame call on `device`: one allocation holding the
 * frame (frame_pixels rows: the path tracer's whole row tiles), the three planes, the result
 * (pixels rows each) and the scratch; finish copies `bytes` of the result to `host` after
 * everything queued on the default stream, and frees. */
typedef struct WoDenoiseWork {
    void* base;
    void *d_color, *d_planes, *d_out, *d_scratch;
} WoDenoiseWork;
int wo_dev_denoise_work_begin(int device, size_t frame_pixels, size_t pixels, size_t scratch_bytes,
                              WoDenoiseWork* work, char* err, size_t errlen);
int wo_dev_denoise_work_finish(WoDenoiseWork* work, void* host, size_t bytes, char* err, size_t errlen);
void wo_dev_denoise_work_free(WoDenoiseWork* work);

#ifdef __cplusplus
}
#endif

#endif /* WOLOLO_WO_DENOISE_H */
