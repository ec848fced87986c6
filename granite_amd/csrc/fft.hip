// Follows MIT-licensed work (Granite, (c) 2015-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// FFT: what renderer/fft/fft.cpp plans and dispatches with fft.comp / fft_r2c.comp / fft_c2r.comp, here one launch per pass of the plan
// of fft_core.hpp.  The arithmetic and the index maps are fft_core.hpp's; this file adds the barriers between the
// phases of a pass, the launches and the checks of what a caller hands in.
//
//   k_fft_pass     a workgroup of 512 lanes holds `columns` adjacent columns of R points in LDS (fp32, padded), runs the radix-4 / radix-8
//                  steps of the R-point transforms in registers with one barrier between a step's reads and its writes, and stores the
//                  tile with the lanes running along memory.  The twiddle of the pass itself is applied on the way in.
//   k_fft_resolve  R2C / C2R: one output column per lane.
#include <new>
#include "ctx.hpp"
#include "fft_core.hpp"

struct gr_fft_plan
{
	gr_fft::Plan plan;
	gr_fft::c32 *twiddle = nullptr;
	uint8_t *scratch[2] = {nullptr, nullptr};
};

namespace
{
using namespace gr_fft;

__global__ __launch_bounds__(GROUP) void k_fft_pass(Pass P)
{
	extern __shared__ c32 lds[];
	c32 regs[REGS];
	const uint32_t lane = threadIdx.x, group = blockIdx.x;
	phase_columns(P, lds, group, lane);
	__syncthreads();
	phase_load(P, lds, group, lane);
	__syncthreads();
	uint32_t local_p = 1;
	for (uint32_t s = 0; s < P.sub_count; s++)
	{
		if (P.sub_radix[s] == 8u)
		{
			phase_butterflies<8>(P, local_p, lds, regs, lane);
			__syncthreads();
			phase_scatter<8>(P, local_p, lds, regs, lane);
			local_p *= 8u;
		}
		else
		{
			phase_butterflies<4>(P, local_p, lds, regs, lane);
			__syncthreads();
			phase_scatter<4>(P, local_p, lds, regs, lane);
			local_p *= 4u;
		}
		__syncthreads();
	}
	phase_store(P, lds, group, lane);
}

__global__ __launch_bounds__(RESOLVE_GROUP) void k_fft_resolve(Pass P)
{
	resolve_element(P, blockIdx.x * RESOLVE_GROUP + threadIdx.x);
}

Options to_options(const gr_fft_options *o)
{
	return {o->nx, o->ny, o->nz, o->dimensions, o->mode, o->data_type, o->input_resource, o->output_resource};
}

uint32_t image_format_of(uint32_t view_kind)
{
	switch (view_kind)
	{
	case VIEW_IMG_C32: return GR_FORMAT_R32G32_SFLOAT;
	case VIEW_IMG_C16: return GR_FORMAT_R16G16_SFLOAT;
	case VIEW_IMG_R32: return GR_FORMAT_R32_SFLOAT;
	default: return GR_FORMAT_R16_SFLOAT;
	}
}

struct Range
{
	uintptr_t first, end;
};

// What execute asks of one side before anything is launched.  Fills the view and the byte range the passes touch.
int check_resource(gr_ctx *ctx, const Options &o, const gr_fft_resource *r, bool output, View &view, Range &range)
{
	const char *what = output ? "dst" : "src";
	if (!r)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: invalid argument: %s is a null pointer", what);
	const uint32_t planned = output ? o.output_resource : o.input_resource;
	if (r->type != planned)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s is resource type %u, the plan was made for %u", what, r->type, planned);
	const uint32_t kind = user_view_kind(o, output);
	if (planned == TEXTURE)
	{
		const gr_image &img = r->image;
		const uint32_t bpp = view_unit_bytes(kind);
		if (img.ptr && img.format != image_format_of(kind))
			return ctx->fail(GR_ERR_UNSUPPORTED_FORMAT, "gr_fft_execute: %s image format %u, this mode and data type store format %u", what, img.format, image_format_of(kind));
		if (const char *rule = gr_image_rule(&img, image_format_of(kind)))
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: invalid argument: %s image%s", what, rule);
		if (img.width > MAX_IMAGE_EXTENT || img.height > MAX_IMAGE_EXTENT)
			return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s image extent %u x %u is outside 1 .. %u", what, img.width, img.height, MAX_IMAGE_EXTENT);
		view = {};
		view.ptr = static_cast<uint8_t *>(img.ptr);
		view.kind = kind;
		view.x_stride = 1;
		view.width = img.width;
		view.height = img.height;
		view.pitch_bytes = img.pitch_bytes;
		view.offset_x = r->output_offset[0];
		view.offset_y = r->output_offset[1];
		range.first = reinterpret_cast<uintptr_t>(img.ptr);
		range.end = range.first + size_t(img.height - 1u) * img.pitch_bytes + size_t(img.width) * bpp;
		return GR_OK;
	}

	const uint32_t unit = view_unit_bytes(kind), row_units = user_row_units(o, output);
	const bool real_side = (kind & 2u) != 0, fp16 = (kind & 1u) != 0;
	if (!r->ptr)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: invalid argument: %s buffer pointer is null", what);
	// a real fp16 side is read and written as whole half2 pairs
	const uint32_t align = (real_side && fp16) ? 4u : unit;
	if (reinterpret_cast<uintptr_t>(r->ptr) % align)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s buffer pointer is not %u-byte aligned", what, align);
	if (real_side && fp16 && ((r->row_stride | r->layer_stride) & 1u))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s strides %u, %u: an FP16 real side needs even strides", what, r->row_stride, r->layer_stride);
	if (o.ny > 1 && r->row_stride < row_units)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s row stride %u is below the %u elements of a row", what, r->row_stride, row_units);
	const uint64_t layer_units = uint64_t(o.ny - 1u) * r->row_stride + row_units;
	if (o.nz > 1 && r->layer_stride < layer_units)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s layer stride %u is below the %llu elements of a layer", what, r->layer_stride, (unsigned long long)layer_units);
	const uint64_t units = uint64_t(o.nz - 1u) * r->layer_stride + layer_units;
	if (units >= (1ull << 31))
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s spans %llu elements, 2^31 or more", what, (unsigned long long)units);
	if (units * unit > r->size_bytes)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: %s needs %llu bytes for its strides, its size is %llu", what, (unsigned long long)(units * unit),
		                 (unsigned long long)r->size_bytes);
	view = linear_view(kind, r->row_stride, r->layer_stride);
	view.ptr = static_cast<uint8_t *>(r->ptr);
	range.first = reinterpret_cast<uintptr_t>(r->ptr);
	range.end = range.first + size_t(r->size_bytes);
	return GR_OK;
}

int launch_pass(gr_ctx *ctx, hipStream_t s, const gr_fft_plan *plan, uint32_t index, const View &src, const View &dst)
{
	Pass P = plan->plan.passes[index];
	auto bind = [&](uint32_t id, View &view) {
		if (id == BUF_SRC)
			view = src;
		else if (id == BUF_DST)
			view = dst;
		else
			view.ptr = plan->scratch[id - BUF_SCRATCH_A];
	};
	bind(P.reads, P.in);
	bind(P.writes, P.out);
	P.twiddle = plan->twiddle;
	if (P.kind == PASS_C2C)
		hipLaunchKernelGGL(k_fft_pass, dim3(P.grid), dim3(GROUP), P.lds_bytes, s, P);
	else
		hipLaunchKernelGGL(k_fft_resolve, dim3(P.grid), dim3(RESOLVE_GROUP), 0, s, P);
	GR_CHECK_LAUNCH(ctx);
	return GR_OK;
}

int execute_range(gr_ctx *ctx, gr_stream stream, const gr_fft_plan *plan, const gr_fft_resource *dst, const gr_fft_resource *src, uint32_t first, uint32_t end)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	if (!plan)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: invalid argument: plan is a null pointer");
	if (end > plan->plan.count)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute_iteration: iteration %u, the plan has %u", end - 1u, plan->plan.count);
	View in, out;
	Range in_range, out_range;
	if (int code = check_resource(ctx, plan->plan.options, src, false, in, in_range))
		return code;
	if (int code = check_resource(ctx, plan->plan.options, dst, true, out, out_range))
		return code;
	if (in_range.first < out_range.end && out_range.first < in_range.end)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute: the source and destination ranges overlap");
	hipStream_t s = gr_to_stream(stream);
	gr_scoped_timing timing{ctx, s, "fft"};
	for (uint32_t i = first; i < end; i++)
		if (int code = launch_pass(ctx, s, plan, i, in, out))
			return code;
	return GR_OK;
}
} // namespace

extern "C" int gr_fft_describe(const gr_fft_options *options, gr_fft_pass *out, uint32_t capacity)
{
	if (!options)
		return GR_ERR_INVALID_ARGUMENT;
	Plan plan;
	if (build_plan(to_options(options), plan) < 0)
		return GR_ERR_INVALID_ARGUMENT;
	for (uint32_t i = 0; i < plan.count && i < capacity && out; i++)
	{
		const Pass &P = plan.passes[i];
		out[i] = {P.kind, P.dim, P.kind == PASS_C2C ? P.radix : 0u, P.kind == PASS_C2C ? P.p : 0u, P.kind == PASS_C2C ? P.columns : 1u, P.group, P.grid, P.lds_bytes, P.reads, P.writes};
	}
	return int(plan.count);
}

extern "C" int gr_fft_plan_create(gr_ctx *ctx, const gr_fft_options *options, gr_fft_plan **out)
{
	if (!ctx)
		return GR_ERR_INVALID_ARGUMENT;
	GR_CHECK_ARG(ctx, options);
	GR_CHECK_ARG(ctx, out);
	*out = nullptr;
	Plan built;
	if (build_plan(to_options(options), built) < 0)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT,
		                 "gr_fft_plan_create: refused: %u x %u x %u, %u dimensions, mode %u, data type %u, input %u, output %u (powers of two of at least 4, or 8 "
		                 "for a real Nx; fewer than 2^31 elements; buffer input; texture output only with Nz = 1 and, for real modes, two dimensions)",
		                 options->nx, options->ny, options->nz, options->dimensions, options->mode, options->data_type, options->input_resource, options->output_resource);
	// tiles above 64 KiB of LDS need the kernel's limit raised; the same value every time
	if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_fft_pass), hipFuncAttributeMaxDynamicSharedMemorySize, int(LDS_LIMIT)) != hipSuccess)
		return ctx->fail(GR_ERR_HIP, "gr_fft_plan_create: the pass kernel's LDS limit could not be set");
	gr_fft_plan *plan = nullptr;
	std::vector<c32> table;
	try
	{
		plan = new gr_fft_plan;
		plan->plan = built;
		table.resize(built.table_n);
	}
	catch (const std::bad_alloc &)
	{
		delete plan;
		return ctx->fail(GR_ERR_OUT_OF_MEMORY, "gr_fft_plan_create: no host memory for the plan and its twiddle table");
	}
	auto fail = [&](int code, const char *what) {
		gr_fft_plan_destroy(ctx, plan);
		return ctx->fail(code, "gr_fft_plan_create: %s", what);
	};
	const Plan &p = plan->plan;
	build_twiddles(table.data(), p.table_n, p.dir);
	if (hipMalloc(reinterpret_cast<void **>(&plan->twiddle), table.size() * sizeof(c32)) != hipSuccess)
		return fail(GR_ERR_OUT_OF_MEMORY, "no memory for the twiddle table");
	if (hipMemcpy(plan->twiddle, table.data(), table.size() * sizeof(c32), hipMemcpyHostToDevice) != hipSuccess)
		return fail(GR_ERR_HIP, "the twiddle table could not be uploaded");
	const size_t scratch_bytes = size_t(p.scratch_elements) * (p.options.data_type == FP16 ? 4u : 8u);
	for (uint32_t i = 0; i < p.scratch_count; i++)
		if (hipMalloc(reinterpret_cast<void **>(&plan->scratch[i]), scratch_bytes) != hipSuccess)
			return fail(GR_ERR_OUT_OF_MEMORY, "no memory for the scratch buffers");
	*out = plan;
	return GR_OK;
}

extern "C" void gr_fft_plan_destroy(gr_ctx *ctx, gr_fft_plan *plan)
{
	(void)ctx;
	if (!plan)
		return;
	(void)hipFree(plan->twiddle);
	(void)hipFree(plan->scratch[0]);
	(void)hipFree(plan->scratch[1]);
	delete plan;
}

extern "C" uint32_t gr_fft_plan_iterations(const gr_fft_plan *plan) { return plan ? plan->plan.count : 0u; }

extern "C" int gr_fft_execute(gr_ctx *ctx, gr_stream stream, const gr_fft_plan *plan, const gr_fft_resource *dst, const gr_fft_resource *src)
{
	return execute_range(ctx, stream, plan, dst, src, 0, plan ? plan->plan.count : 0u);
}

extern "C" int gr_fft_execute_iteration(gr_ctx *ctx, gr_stream stream, const gr_fft_plan *plan, const gr_fft_resource *dst, const gr_fft_resource *src,
                                        uint32_t iteration)
{
	if (ctx && plan && iteration >= plan->plan.count)
		return ctx->fail(GR_ERR_INVALID_ARGUMENT, "gr_fft_execute_iteration: iteration %u, the plan has %u", iteration, plan->plan.count);
	return execute_range(ctx, stream, plan, dst, src, iteration, iteration + 1u);
}
