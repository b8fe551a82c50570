// jpeg_encode_color.hip -- an 8-bit RGB or grey image -> the padded component planes of a JPEG encode (include/mdct_jpegenc.h):
// libjpeg-turbo's integer RGB -> YCbCr (jccolor.c), its chroma downsampling (jcsample.c) and edge padding to the block grid, bit for
// bit.
//
// Built into its own library, libmdct_jpegenc.so, linked against libmdct_hip.so (whose launch tally counts its launches).  One kernel
// template, k_rgb_ycc<Kind, Planar>: a workgroup per tile of 1024 luma columns x 4 row groups, the image's record in the kernel
// arguments.  The tile itself -- the vector path, the LDS staging, the scalar rule -- and the host checks are rgb_ycc.h's, shared with
// the batch encoder (jpeg_encode_batch.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegenc.h"
#include "rgb_ycc.h"

namespace mdct
{
namespace jpegenc
{

template <int Kind, bool Planar>
__global__ __launch_bounds__(kWG) void k_rgb_ycc(EncArgs a)
{
  __shared__ uint4 lds[kStageSlots<Kind, Planar>];
  rgb_ycc_tile<Kind, Planar>(a, (int)blockIdx.x, (int)blockIdx.y, lds);
}

} // namespace jpegenc
} // namespace mdct

using namespace mdct::jpegenc;

namespace
{

template <int Kind>
void launch(bool planar, dim3 grid, hipStream_t s, const EncArgs &a)
{
  if (planar)
    MDCT_LAUNCH((k_rgb_ycc<Kind, true>), grid, dim3(kWG), 0, s, a);
  else
    MDCT_LAUNCH((k_rgb_ycc<Kind, false>), grid, dim3(kWG), 0, s, a);
}

} // namespace

extern "C" {

const char *mdct_jpegenc_last_error(void) { return g_err; }

int mdct_jpegenc_from_rgb(const uint8_t *in, size_t in_pitch, size_t in_plane_stride, size_t width, size_t height, int colour, int layout,
                          const mdct_jpegenc_plane *planes, int n_planes, void *stream)
{
  EncArgs a;
  int kind;
  bool planar;
  const int rc = check_rgb_image(in, in_pitch, in_plane_stride, width, height, colour, layout, planes, n_planes, a, &kind, &planar);
  if (rc)
    return rc;
  const dim3 grid((unsigned)((a.X + 64 * kRun - 1) / (64 * kRun)), (unsigned)((a.G + kRows - 1) / kRows));
  const hipStream_t s = (hipStream_t)stream;
  switch (kind)
  {
  case kGrey: MDCT_LAUNCH((k_rgb_ycc<kGrey, false>), grid, dim3(kWG), 0, s, a); break;
  case k444: launch<k444>(planar, grid, s, a); break;
  case k422: launch<k422>(planar, grid, s, a); break;
  default: launch<k420>(planar, grid, s, a); break;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // extern "C"
