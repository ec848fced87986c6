// TEST INFRASTRUCTURE.  granite_amd/csrc/fft_core.hpp -- the plan, the index maps and the butterflies the kernels of fft.hip call --
// built for the host as a shared library.  A plan made by build_plan is executed pass by pass as the kernels execute it: every
// workgroup of every pass, its 512 lanes one at a time through each phase, with the registers a lane keeps across the barrier between
// a step's reads and its writes held per lane.  tests/test_fft_core_cpu.py holds the result to numpy's float64 DFT before a device sees
// the code.
#include <vector>
#include "../../granite_amd/csrc/fft_core.hpp"

using namespace gr_fft;

namespace
{
void run_pass(const Pass &P)
{
	if (P.kind != PASS_C2C)
	{
		for (uint32_t group = 0; group < P.grid; group++)
			for (uint32_t lane = 0; lane < RESOLVE_GROUP; lane++)
				resolve_element(P, group * RESOLVE_GROUP + lane);
		return;
	}
	std::vector<c32> lds(P.lds_bytes / sizeof(c32) + 1u);
	std::vector<c32> regs(size_t(GROUP) * REGS);
	for (uint32_t group = 0; group < P.grid; group++)
	{
		for (uint32_t lane = 0; lane < GROUP; lane++)
			phase_columns(P, lds.data(), group, lane);
		for (uint32_t lane = 0; lane < GROUP; lane++)
			phase_load(P, lds.data(), group, lane);
		uint32_t local_p = 1;
		for (uint32_t s = 0; s < P.sub_count; s++)
		{
			const bool eight = P.sub_radix[s] == 8u;
			for (uint32_t lane = 0; lane < GROUP; lane++)
			{
				if (eight)
					phase_butterflies<8>(P, local_p, lds.data(), &regs[size_t(lane) * REGS], lane);
				else
					phase_butterflies<4>(P, local_p, lds.data(), &regs[size_t(lane) * REGS], lane);
			}
			for (uint32_t lane = 0; lane < GROUP; lane++)
			{
				if (eight)
					phase_scatter<8>(P, local_p, lds.data(), &regs[size_t(lane) * REGS], lane);
				else
					phase_scatter<4>(P, local_p, lds.data(), &regs[size_t(lane) * REGS], lane);
			}
			local_p *= P.sub_radix[s];
		}
		for (uint32_t lane = 0; lane < GROUP; lane++)
			phase_store(P, lds.data(), group, lane);
	}
}
} // namespace

// dst / src: host memory laid out as the device buffers are.  image: {width, height, pitch_bytes, offset_x, offset_y} for texture output.
extern "C" int fft_host_execute(const Options *options, void *dst, uint32_t dst_row_stride, uint32_t dst_layer_stride, const void *src, uint32_t src_row_stride,
                                uint32_t src_layer_stride, const int32_t *image)
{
	Plan plan;
	if (build_plan(*options, plan) < 0)
		return -1;
	std::vector<c32> table(plan.table_n);
	build_twiddles(table.data(), plan.table_n, plan.dir);
	const size_t scratch_bytes = size_t(plan.scratch_elements) * (options->data_type == FP16 ? 4u : 8u);
	std::vector<uint8_t> scratch[2];
	for (uint32_t i = 0; i < plan.scratch_count; i++)
		scratch[i].assign(scratch_bytes, 0);
	View in = linear_view(user_view_kind(*options, false), src_row_stride, src_layer_stride);
	in.ptr = static_cast<uint8_t *>(const_cast<void *>(src));
	View out = linear_view(user_view_kind(*options, true), dst_row_stride, dst_layer_stride);
	out.ptr = static_cast<uint8_t *>(dst);
	if (options->output_resource == TEXTURE)
	{
		out.x_stride = 1;
		out.width = uint32_t(image[0]);
		out.height = uint32_t(image[1]);
		out.pitch_bytes = uint32_t(image[2]);
		out.offset_x = image[3];
		out.offset_y = image[4];
	}
	for (uint32_t i = 0; i < plan.count; i++)
	{
		Pass P = plan.passes[i];
		auto bind = [&](uint32_t id, View &view) {
			if (id == BUF_SRC)
				view = in;
			else if (id == BUF_DST)
				view = out;
			else
				view.ptr = scratch[id - BUF_SCRATCH_A].data();
		};
		bind(P.reads, P.in);
		bind(P.writes, P.out);
		P.twiddle = table.data();
		run_pass(P);
	}
	return int(plan.count);
}
