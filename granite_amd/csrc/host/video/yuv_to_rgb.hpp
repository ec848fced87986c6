// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The conversion half of Granite::VideoDecoder (video/ffmpeg_decode.cpp: init_yuv_to_rgb, dispatch_conversion) on the HIP executor,
// without the decoder: planes are gr_image descriptors instead of image views, the UBO and the specialization constants are the
// library's plan (gr_video_yuv_plan) and the program is the library's own (gr_video_yuv_to_rgb, csrc/video.hip).
#pragma once
#include "../../../../include/granite_hip.h"

namespace Granite
{
class VideoYuvToRgb
{
public:
	// What init_yuv_to_rgb decides once per stream: checks plane and output shapes (pointers are not read) and keeps the plan.
	// Throws std::logic_error when the conversion is not supported.
	void init(const gr_image *planes, unsigned num_planes, const gr_image &output, const gr_video_yuv_info &info);
	// dispatch_conversion: planes and output of the shapes given to init.  Throws std::runtime_error with gr_last_error's message when
	// the launcher refuses.
	void convert(gr_ctx *ctx, gr_stream stream, const gr_image *planes, const gr_image &output) const;

	const struct gr_video_yuv_plan &get_plan() const { return plan; }
	unsigned get_num_planes() const { return num_planes; }

private:
	struct gr_video_yuv_plan plan = {};
	gr_video_yuv_info info = {};
	unsigned num_planes = 0;
};
} // namespace Granite
