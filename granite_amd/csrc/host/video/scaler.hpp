// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Granite::VideoScaler (video/scaler.hpp) on the HIP executor: RescaleInfo names gr_image planes instead of image views, and the
// program is the library's own (gr_video_scale, csrc/video.hip), so set_program is gone.  The launcher keeps the weight table.
#pragma once
#include "../../../../include/granite_hip.h"

namespace Granite
{
class VideoScaler
{
public:
	struct RescaleInfo
	{
		const gr_image *output_planes[3];
		unsigned num_output_planes;
		const gr_image *input;
		uint32_t input_color_space;  // VkColorSpaceKHR values (GR_COLOR_SPACE_*)
		uint32_t output_color_space;
	};

	// Throws std::runtime_error with gr_last_error's message when the launcher refuses.
	void rescale(gr_ctx *ctx, gr_stream stream, const RescaleInfo &info);
	void reset() {}
};
} // namespace Granite
