// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "shadow.hpp"
#include <stdexcept>

namespace Granite
{
void setup_vsm_chain(gr_ctx *ctx, gr_stream stream, const VsmChainLayer *layers, unsigned count)
{
	auto check = [&](int status) {
		if (status < 0)
			throw std::runtime_error(gr_last_error(ctx));
	};
	for (unsigned i = 0; i < count; i++)
	{
		const VsmChainLayer &l = layers[i];
		check(gr_vsm_moments(ctx, stream, &l.depth->get_view(), &l.raw->get_view()));
		check(gr_vsm_blur(ctx, stream, &l.raw->get_view(), &l.half->get_view(), 0));
		check(gr_vsm_blur(ctx, stream, &l.half->get_view(), &l.blurred->get_view(), 1));
	}
}
} // namespace Granite
