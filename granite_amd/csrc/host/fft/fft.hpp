// Follows MIT-licensed work (Granite, (c) 2015-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Granite::FFT (renderer/fft/fft.hpp) on the HIP executor: the reference's class surface over HIP::Device, its buffers and image views;
// the command buffer's stream takes the place of the Vulkan command buffer.  The plan, the kernels and every check are the library's
// (gr_fft_*, csrc/fft.hip).  Texture input is refused by plan().  A planned FFT may be in flight on one stream at a time.
#pragma once
#include "../hip_device.hpp"

namespace Granite
{
class FFT
{
public:
	FFT() = default;
	~FFT();
	FFT(const FFT &) = delete;
	void operator=(const FFT &) = delete;

	enum class ResourceType { Texture, Buffer };
	enum class Mode { ForwardComplexToComplex, InverseComplexToComplex, RealToComplex, ComplexToReal };
	enum class DataType { FP32, FP16 };

	struct Options
	{
		unsigned Nx = 1;
		unsigned Ny = 1;
		unsigned Nz = 1;
		ResourceType input_resource = ResourceType::Buffer;
		ResourceType output_resource = ResourceType::Buffer;
		Mode mode = Mode::ForwardComplexToComplex;
		DataType data_type = DataType::FP32;
		// If Ny or Nz are larger than 1 and dimensions is smaller than 2 or 3 respectively, the transforms are batched.
		unsigned dimensions = 1;
	};

	struct BufferResource
	{
		const HIP::Buffer *buffer;
		size_t offset;
		size_t size;
		// In elements: scalars on a real side, complex numbers otherwise; even on an FP16 real side.
		uint32_t row_stride;
		uint32_t layer_stride;
	};

	struct ImageResource
	{
		const HIP::ImageView *view;
		int32_t output_offset[2];
	};

	union Resource
	{
		BufferResource buffer;
		ImageResource image;
	};

	// false where the reference's plan() returns false, for texture input and for 2^31 elements or more (gr_last_error has the reason).
	bool plan(HIP::Device *device, const Options &options);
	// Throws std::runtime_error with gr_last_error's message when the library refuses the resources, std::logic_error without a plan or
	// for a buffer range outside its buffer; nothing is launched then.
	void execute(HIP::CommandBuffer &cmd, const Resource &dst, const Resource &src);
	void execute_iteration(HIP::CommandBuffer &cmd, const Resource &dst, const Resource &src, unsigned iteration);
	unsigned get_num_iterations() const;
	void release();

private:
	HIP::Device *device = nullptr;
	Options options;
	gr_fft_plan *handle = nullptr;
};
} // namespace Granite
