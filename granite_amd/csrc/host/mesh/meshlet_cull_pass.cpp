// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// build_mdi_culling_pass (renderer/scene_renderer.cpp:954-1035) for one context: the launches.  What each launch is given is
// describe_mdi_cull's, in meshlet_cull.cpp.
#include "meshlet_cull.hpp"

namespace Granite
{
bool build_mdi_culling_pass(gr_ctx *ctx, gr_stream stream, const CullingContext &context, CullingPhase phase, bool force_visible, uint32_t width, uint32_t height,
                            const std::vector<MDICall> &calls)
{
	for (const MDICall &call : calls)
	{
		if (call.indirect_count_max == 0u)
			continue;
		gr_meshlet_cull_args args;
		gr_push_meshlet_cull push;
		describe_mdi_cull(context, phase, force_visible, width, height, call, args, push);
		if (gr_meshlet_cull(ctx, stream, &args, &push) != GR_OK)
			return false;
	}
	return true;
}
} // namespace Granite
