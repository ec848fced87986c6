// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "scaler.hpp"
#include <stdexcept>
#include <string>

namespace Granite
{
void VideoScaler::rescale(gr_ctx *ctx, gr_stream stream, const RescaleInfo &info)
{
	if (!info.input || info.num_output_planes < 1 || info.num_output_planes > 3)
		throw std::logic_error("VideoScaler::rescale: input and one to three output planes are required");
	gr_image planes[3] = {};
	for (unsigned i = 0; i < info.num_output_planes; i++)
	{
		if (!info.output_planes[i])
			throw std::logic_error("VideoScaler::rescale: missing output plane");
		planes[i] = *info.output_planes[i];
	}
	if (gr_video_scale(ctx, stream, info.input, planes, info.num_output_planes, info.input_color_space, info.output_color_space) < 0)
		throw std::runtime_error(std::string("VideoScaler::rescale: ") + gr_last_error(ctx));
}
} // namespace Granite
