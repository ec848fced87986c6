// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "yuv_to_rgb.hpp"
#include <stdexcept>
#include <string>

namespace Granite
{
void VideoYuvToRgb::init(const gr_image *planes, unsigned count, const gr_image &output, const gr_video_yuv_info &stream_info)
{
	if (gr_video_yuv_plan(planes, count, &output, &stream_info, &plan) < 0)
		throw std::logic_error("VideoYuvToRgb::init: the conversion is not supported for these planes, this output format and this stream description");
	info = stream_info;
	num_planes = count;
}

void VideoYuvToRgb::convert(gr_ctx *ctx, gr_stream stream, const gr_image *planes, const gr_image &output) const
{
	if (!num_planes)
		throw std::logic_error("VideoYuvToRgb::convert: init() has not run");
	if (gr_video_yuv_to_rgb(ctx, stream, planes, num_planes, &output, &info) < 0)
		throw std::runtime_error(std::string("VideoYuvToRgb::convert: ") + gr_last_error(ctx));
}
} // namespace Granite
