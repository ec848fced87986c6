// Follows MIT-licensed work (Granite, (c) 2015-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "fft.hpp"
#include <stdexcept>
#include <string>

namespace Granite
{
namespace
{
gr_fft_resource to_resource(FFT::ResourceType type, const FFT::Resource &r)
{
	gr_fft_resource out = {};
	if (type == FFT::ResourceType::Buffer)
	{
		out.type = GR_FFT_RESOURCE_BUFFER;
		// the stated range is what the library trusts: it has to lie inside the buffer
		if (r.buffer.buffer && (r.buffer.offset > r.buffer.buffer->get_size() || r.buffer.size > r.buffer.buffer->get_size() - r.buffer.offset))
			throw std::logic_error("Granite::FFT: buffer resource offset + size lies outside the buffer");
		out.ptr = r.buffer.buffer ? static_cast<uint8_t *>(r.buffer.buffer->get_device_pointer()) + r.buffer.offset : nullptr;
		out.size_bytes = r.buffer.size;
		out.row_stride = r.buffer.row_stride;
		out.layer_stride = r.buffer.layer_stride;
	}
	else
	{
		out.type = GR_FFT_RESOURCE_TEXTURE;
		if (r.image.view)
			out.image = r.image.view->get_view();
		out.output_offset[0] = r.image.output_offset[0];
		out.output_offset[1] = r.image.output_offset[1];
	}
	return out;
}
} // namespace

FFT::~FFT() { release(); }

void FFT::release()
{
	if (handle)
		gr_fft_plan_destroy(device->get_context(), handle);
	handle = nullptr;
	device = nullptr;
}

bool FFT::plan(HIP::Device *device_, const Options &options_)
{
	release();
	device = device_;
	options = options_;
	device->make_current();
	gr_fft_options o = {};
	o.nx = options.Nx;
	o.ny = options.Ny;
	o.nz = options.Nz;
	o.dimensions = options.dimensions;
	o.mode = uint32_t(options.mode);
	o.data_type = uint32_t(options.data_type);
	o.input_resource = uint32_t(options.input_resource);
	o.output_resource = uint32_t(options.output_resource);
	if (gr_fft_plan_create(device->get_context(), &o, &handle) != GR_OK)
	{
		handle = nullptr;
		return false;
	}
	return true;
}

void FFT::execute(HIP::CommandBuffer &cmd, const Resource &dst, const Resource &src)
{
	if (!handle)
		throw std::logic_error("Granite::FFT: execute without a plan");
	const gr_fft_resource d = to_resource(options.output_resource, dst), s = to_resource(options.input_resource, src);
	if (gr_fft_execute(cmd.get_context(), cmd.get_stream(), handle, &d, &s) != GR_OK)
		throw std::runtime_error(std::string("Granite::FFT::execute: ") + gr_last_error(cmd.get_context()));
}

void FFT::execute_iteration(HIP::CommandBuffer &cmd, const Resource &dst, const Resource &src, unsigned iteration)
{
	if (!handle)
		throw std::logic_error("Granite::FFT: execute without a plan");
	const gr_fft_resource d = to_resource(options.output_resource, dst), s = to_resource(options.input_resource, src);
	if (gr_fft_execute_iteration(cmd.get_context(), cmd.get_stream(), handle, &d, &s, iteration) != GR_OK)
		throw std::runtime_error(std::string("Granite::FFT::execute_iteration: ") + gr_last_error(cmd.get_context()));
}

unsigned FFT::get_num_iterations() const { return handle ? gr_fft_plan_iterations(handle) : 0u; }
} // namespace Granite
