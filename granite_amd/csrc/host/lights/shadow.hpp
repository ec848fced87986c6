// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// The directional light's VSM chain as the scene viewer's graph runs it (scene_viewer_application.cpp:1085-1131): "shadow-raw" (moments, the
// shadow map's size), "shadow-down" (half size) and "shadow" (the map's size again), every layer of the map.
#pragma once
#include "../hip_device.hpp"

namespace Granite
{
// The middle image of the chain along one axis.  The graph declares it as an absolute size, `size_x *= 0.5f`, and an absolute size is
// converted to unsigned -- truncated, not rounded up as a relative size is -- and is at least 1 (render_graph.cpp: SizeClass::Absolute).
inline unsigned vsm_half_size(unsigned size)
{
	const unsigned half = unsigned(float(size) * 0.5f);
	return half ? half : 1u;
}

// The three images of one layer; `raw` and `blurred` have the depth layer's size, `half` has vsm_half_size of it each way.
struct VsmChainLayer
{
	const HIP::Image *depth; // D16_UNORM or D32_SFLOAT
	HIP::Image *raw, *half, *blurred;
};

// moments -> down blur -> up blur over all layers, recorded on `stream`.  The reference resolves a 4x MSAA target into "shadow-raw"; nothing
// is rasterised here, so the moments are those of the one depth value a texel has.  Throws what a launcher refuses.
void setup_vsm_chain(gr_ctx *ctx, gr_stream stream, const VsmChainLayer *layers, unsigned count);
} // namespace Granite
