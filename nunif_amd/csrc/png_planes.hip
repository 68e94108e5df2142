// The plane forms of the PNG frame encoder (png.hip): RGBA 8, grey 8 and grey + alpha 8 from planar fp32 colour and a separate
// planar fp32 alpha, as Waifu2x.convert returns them (waifu2x/ui_utils.py:42-100 process_image, nunif/utils/pil_io.py:240-323
// to_image / save_image, reference).  Only the first launch knows the form; this file instantiates it for the three of them.
#include "png_filter.h"

namespace nunif {
namespace png_dev {

int launch_filter_planes(const void *src, const Planes &pl, const Frame &f, uint8_t *filt, uint32_t *rowsum, long frame_stride,
                         hipStream_t s) {
    const dim3 grid(cdiv(f.H, 4), f.B);
    if (f.form == kRgba8F32) png_filter_kernel<kRgba8F32><<<grid, kThreads, 0, s>>>(src, pl, filt, rowsum, f, frame_stride);
    else if (f.form == kGray8F32) png_filter_kernel<kGray8F32><<<grid, kThreads, 0, s>>>(src, pl, filt, rowsum, f, frame_stride);
    else if (f.form == kGrayA8F32) png_filter_kernel<kGrayA8F32><<<grid, kThreads, 0, s>>>(src, pl, filt, rowsum, f, frame_stride);
    else NUNIF_REQUIRE(false, "png: form %d has no planes", f.form);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

}  // namespace png_dev
}  // namespace nunif
