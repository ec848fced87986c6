// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
#include "ocean.hpp"
#include "post/spd.hpp"
#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace Granite
{
namespace
{
constexpr double AnimationPeriod = 256.0;
constexpr double AnimationPeriodScaled = AnimationPeriod / (2.0 * 3.14159265358979323846);
constexpr float TwoPi = 6.28318530717958647692f;

enum : unsigned
{
	HeightInput = 0,
	NormalInput,
	DisplacementInput,
	HeightOutput,
	DisplacementOutput,
	NormalOutput,
	SpdCounter,
	GradientJacobian,
	HeightDisplacement,
	Lods,
	LodCounter,
	LodData
};

OceanLodRequest checked(const OceanConfig &config, const OceanLodRequest &request)
{
	if (request.lod_update)
		OceanLod::check_lod_update(config);
	return request;
}

std::vector<gr_image> level_views(const HIP::Image &image, unsigned levels)
{
	std::vector<gr_image> views;
	for (unsigned i = 0; i < levels; i++)
		views.push_back(image.get_level_view(i));
	return views;
}
} // namespace

const char *const Ocean::ResourceNames[Ocean::TotalResourceCount] = {
	"ocean-height-fft-input",  "ocean-normal-fft-input",  "ocean-displacement-fft-input",
	"ocean-height-fft-output", "ocean-displacement-fft-output", "ocean-normal-fft-output",
	"ocean-spd-counter",       "ocean-gradient-jacobian-output", "ocean-height-displacement-output",
	"ocean-lods",              "ocean-lod-counter",       "ocean-lod-data",
};

Ocean::Ocean(const OceanConfig &config, bool force_mipmap_shader_, const OceanLodRequest &lod_request_)
	: parameters(derive_ocean_parameters(config)), force_mipmap_shader(force_mipmap_shader_), lod_request(checked(config, lod_request_)),
	  lod(parameters.config, lod_request_.fixed_position, lod_request_.center_position)
{
	for (auto &f : frequency_bands)
		f = 1.0f;
}

Ocean::~Ocean()
{
	if (device)
		device->wait_idle();
}

void Ocean::set_frequency_band_amplitude(unsigned band, float amplitude)
{
	if (band >= FrequencyBands)
		throw std::out_of_range("Ocean: frequency band out of range.");
	frequency_bands[band] = amplitude;
}

void Ocean::on_device_created(HIP::Device &device_)
{
	device = &device_;
	auto &config = parameters.config;
	FFT::Options options;
	options.data_type = FFT::DataType::FP16;
	options.dimensions = 2;
	options.input_resource = FFT::ResourceType::Buffer;
	options.output_resource = FFT::ResourceType::Texture;

	options.mode = FFT::Mode::ComplexToReal;
	options.Nx = options.Ny = config.fft_resolution;
	bool planned = height_fft.plan(device, options);
	options.mode = FFT::Mode::InverseComplexToComplex;
	planned = planned && normal_fft.plan(device, options);
	options.Nx = options.Ny = config.fft_resolution >> config.displacement_downsample;
	planned = planned && displacement_fft.plan(device, options);
	if (!planned)
		throw std::runtime_error(std::string("Ocean: failed to plan FFT: ") + gr_last_error(device->get_context()));
	init_distributions(device_);
	if (lod_request.lod_update)
		build_buffers(device_);
}

void Ocean::build_buffers(HIP::Device &device_)
{
	gr_ctx *ctx = device_.get_context();
	auto upload = [&](const void *data, size_t size, VkBufferUsageFlags usage, const char *name) {
		auto buffer = device_.create_buffer(size, usage, name);
		if (gr_upload(ctx, nullptr, buffer->get_device_pointer(), data, size) < 0 || gr_sync(ctx, nullptr) < 0)
			throw std::runtime_error(std::string("Ocean: mesh upload: ") + gr_last_error(ctx));
		return buffer;
	};
	for (unsigned i = 0; i < lod.get_lod_count(); i++)
	{
		const OceanLodMesh &mesh = lod.get_lod_mesh(i);
		lod_vbos.push_back(upload(mesh.vertices.data(), mesh.vertices.size() * sizeof(OceanVertex), VK_BUFFER_USAGE_VERTEX_BUFFER_BIT, "ocean-lod-vbo"));
		lod_ibos.push_back(upload(mesh.indices.data(), mesh.indices.size() * sizeof(uint16_t), VK_BUFFER_USAGE_INDEX_BUFFER_BIT, "ocean-lod-ibo"));
	}
	const OceanBorderMesh &border = lod.get_border_mesh();
	if (!border.positions.empty())
	{
		border_vbo = upload(border.positions.data(), border.positions.size() * sizeof(vec3), VK_BUFFER_USAGE_VERTEX_BUFFER_BIT, "ocean-border-vbo");
		border_ibo = upload(border.indices.data(), border.indices.size() * sizeof(uint16_t), VK_BUFFER_USAGE_INDEX_BUFFER_BIT, "ocean-border-ibo");
	}
}

void Ocean::add_lod_update_pass(RenderGraph &graph_)
{
	if (!lod_request.lod_update)
		throw std::logic_error("Ocean: add_lod_update_pass on an ocean created without a LOD request.");
	graph = &graph_;
	const unsigned count = parameters.config.grid_count;
	auto &update_lod = graph_.add_pass("ocean-update-lods", RENDER_GRAPH_QUEUE_COMPUTE_BIT);
	AttachmentInfo lod_attachment;
	lod_attachment.format = VK_FORMAT_R16_SFLOAT;
	lod_attachment.size_x = lod_attachment.size_y = float(count);
	lod_attachment.size_class = SizeClass::Absolute;
	graph_textures[Lods] = &update_lod.add_storage_texture_output(ResourceNames[Lods], lod_attachment);

	BufferInfo lod_info_counter, lod_info;
	lod_info_counter.size = OceanLod::MaxLODIndirect * sizeof(gr_ocean_indirect_draw);
	lod_info_counter.usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_INDIRECT_BUFFER_BIT;
	graph_buffers[LodCounter] = &update_lod.add_storage_output(ResourceNames[LodCounter], lod_info_counter);
	lod_info.size = VkDeviceSize(count) * count * OceanLod::MaxLODIndirect * sizeof(gr_ocean_patch);
	lod_info.usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT;
	graph_buffers[LodData] = &update_lod.add_storage_output(ResourceNames[LodData], lod_info);
	update_lod.set_build_render_pass([this](HIP::CommandBuffer &cmd) { update_lod_pass(cmd); });
}

void Ocean::init_distributions(HIP::Device &device_)
{
	distributions = make_ocean_distributions(parameters);
	gr_ctx *ctx = device_.get_context();
	auto upload = [&](const std::vector<vec2> &host, const char *name) {
		auto buffer = device_.create_buffer(host.size() * sizeof(vec2), VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, name);
		if (gr_upload(ctx, nullptr, buffer->get_device_pointer(), host.data(), host.size() * sizeof(vec2)) < 0 || gr_sync(ctx, nullptr) < 0)
			throw std::runtime_error(std::string("Ocean: distribution upload: ") + gr_last_error(ctx));
		return buffer;
	};
	distribution_buffer = upload(distributions.height, "ocean-distribution-height");
	distribution_buffer_displacement = upload(distributions.displacement, "ocean-distribution-displacement");
	distribution_buffer_normal = upload(distributions.normal, "ocean-distribution-normal");
}

void Ocean::add_fft_update_pass(RenderGraph &graph_)
{
	graph = &graph_;
	auto &config = parameters.config;
	const unsigned n = config.fft_resolution, m = n >> config.displacement_downsample;

	BufferInfo full_info, displacement_info;
	full_info.size = VkDeviceSize(n) * n * sizeof(uint32_t);
	full_info.usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT;
	displacement_info.size = VkDeviceSize(m) * m * sizeof(uint32_t);
	displacement_info.usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT;

	AttachmentInfo normal_map, displacement_map, height_map;
	normal_map.size_class = displacement_map.size_class = height_map.size_class = SizeClass::Absolute;
	normal_map.size_x = normal_map.size_y = float(n);
	normal_map.format = VK_FORMAT_R16G16_SFLOAT;
	normal_map.levels = 0; // the full chain
	displacement_map.size_x = displacement_map.size_y = float(m);
	displacement_map.format = VK_FORMAT_R16G16_SFLOAT;
	height_map.size_x = height_map.size_y = float(n);
	height_map.format = VK_FORMAT_R16_SFLOAT;

	auto &update_fft = graph_.add_pass("ocean-update-fft", RENDER_GRAPH_QUEUE_COMPUTE_BIT);
	graph_buffers[HeightInput] = &update_fft.add_storage_output(ResourceNames[HeightInput], full_info);
	graph_buffers[NormalInput] = &update_fft.add_storage_output(ResourceNames[NormalInput], full_info);
	graph_buffers[DisplacementInput] = &update_fft.add_storage_output(ResourceNames[DisplacementInput], displacement_info);
	graph_textures[HeightOutput] = &update_fft.add_storage_texture_output(ResourceNames[HeightOutput], height_map);
	graph_textures[NormalOutput] = &update_fft.add_storage_texture_output(ResourceNames[NormalOutput], normal_map);
	graph_textures[DisplacementOutput] = &update_fft.add_storage_texture_output(ResourceNames[DisplacementOutput], displacement_map);

	BufferInfo spd_info;
	spd_info.size = 3 * 4; // three tickets of the shader's; the downsampler here does not use them
	spd_info.usage = VK_BUFFER_USAGE_STORAGE_BUFFER_BIT;
	graph_buffers[SpdCounter] = &update_fft.add_storage_output(ResourceNames[SpdCounter], spd_info);

	AttachmentInfo height_displacement;
	height_displacement.size_class = SizeClass::Absolute;
	height_displacement.size_x = height_displacement.size_y = float(n);
	height_displacement.format = VK_FORMAT_R16G16B16A16_SFLOAT;
	height_displacement.levels = parameters.vertex_levels();
	if (config.heightmap)
		graph_textures[HeightDisplacement] = &update_fft.add_storage_texture_output(ResourceNames[HeightDisplacement], height_displacement);
	height_displacement.levels = 0;
	graph_textures[GradientJacobian] = &update_fft.add_storage_texture_output(ResourceNames[GradientJacobian], height_displacement);

	update_fft.set_build_render_pass([this](HIP::CommandBuffer &cmd) { update_fft_pass(cmd); });
}

void Ocean::create_resources(HIP::Device &device_)
{
	graph = nullptr;
	auto &config = parameters.config;
	const unsigned n = config.fft_resolution, m = n >> config.displacement_downsample;
	unsigned full = 1;
	while ((n >> full) != 0)
		full++;
	own_buffers[HeightInput] = device_.create_buffer(size_t(n) * n * 4, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, ResourceNames[HeightInput]);
	own_buffers[NormalInput] = device_.create_buffer(size_t(n) * n * 4, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, ResourceNames[NormalInput]);
	own_buffers[DisplacementInput] = device_.create_buffer(size_t(m) * m * 4, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, ResourceNames[DisplacementInput]);
	own_buffers[SpdCounter] = device_.create_buffer(3 * 4, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, ResourceNames[SpdCounter]);
	own_images[HeightOutput] = device_.create_image(n, n, VK_FORMAT_R16_SFLOAT, ResourceNames[HeightOutput]);
	own_images[DisplacementOutput] = device_.create_image(m, m, VK_FORMAT_R16G16_SFLOAT, ResourceNames[DisplacementOutput]);
	own_images[NormalOutput] = device_.create_image(n, n, VK_FORMAT_R16G16_SFLOAT, ResourceNames[NormalOutput], full);
	own_images[GradientJacobian] = device_.create_image(n, n, VK_FORMAT_R16G16B16A16_SFLOAT, ResourceNames[GradientJacobian], full);
	if (config.heightmap)
		own_images[HeightDisplacement] =
				device_.create_image(n, n, VK_FORMAT_R16G16B16A16_SFLOAT, ResourceNames[HeightDisplacement], std::max(parameters.vertex_levels(), 1u));
	if (lod_request.lod_update)
	{
		const unsigned count = config.grid_count;
		own_images[Lods] = device_.create_image(count, count, VK_FORMAT_R16_SFLOAT, ResourceNames[Lods]);
		own_buffers[LodCounter] = device_.create_buffer(OceanLod::MaxLODIndirect * sizeof(gr_ocean_indirect_draw),
		                                                VK_BUFFER_USAGE_STORAGE_BUFFER_BIT | VK_BUFFER_USAGE_INDIRECT_BUFFER_BIT, ResourceNames[LodCounter]);
		own_buffers[LodData] = device_.create_buffer(size_t(count) * count * OceanLod::MaxLODIndirect * sizeof(gr_ocean_patch), VK_BUFFER_USAGE_STORAGE_BUFFER_BIT,
		                                             ResourceNames[LodData]);
	}
}

HIP::Buffer *Ocean::get_buffer(unsigned which)
{
	if (which >= TotalResourceCount)
		return nullptr;
	if (graph)
		return graph_buffers[which] ? graph->maybe_get_physical_buffer_resource(graph_buffers[which]) : nullptr;
	return own_buffers[which].get();
}

HIP::Image *Ocean::get_image(unsigned which)
{
	if (which >= TotalResourceCount)
		return nullptr;
	if (graph)
		return graph_textures[which] ? graph->maybe_get_physical_texture_resource(graph_textures[which]) : nullptr;
	return own_images[which].get();
}

unsigned Ocean::get_levels(unsigned which)
{
	HIP::Image *image = get_image(which);
	if (!image)
		return 0;
	if (which == HeightDisplacement)
		return std::min(std::max(parameters.vertex_levels(), 1u), image->get_levels());
	return image->get_levels();
}

void Ocean::update_fft_input(HIP::CommandBuffer &cmd)
{
	auto &config = parameters.config;
	const unsigned n = config.fft_resolution, m = n >> config.displacement_downsample;
	const vec2 world = heightmap_world_size(), normal_world = normalmap_world_size();
	gr_push_ocean_generate push = {};
	push.mod_factor[0] = TwoPi / world.x;
	push.mod_factor[1] = TwoPi / world.y;
	push.time = float(std::fmod(elapsed_time, AnimationPeriod));
	push.period = float(AnimationPeriodScaled);
	push.freq_to_band_mod = (float(FrequencyBands - 1) * 2.0f) / float(n);
	const float *bands = freq_band_modulation ? frequency_bands : nullptr;

	push.N[0] = push.N[1] = n;
	cmd.check(gr_ocean_generate_fft(cmd.get_context(), cmd.get_stream(), distribution_buffer->get_device_pointer(),
	                                get_buffer(HeightInput)->get_device_pointer(), &push, GR_OCEAN_VARIANT_HEIGHT, bands),
	          "ocean height spectrum");
	push.N[0] = push.N[1] = m;
	cmd.check(gr_ocean_generate_fft(cmd.get_context(), cmd.get_stream(), distribution_buffer_displacement->get_device_pointer(),
	                                get_buffer(DisplacementInput)->get_device_pointer(), &push, GR_OCEAN_VARIANT_GRADIENT_DISPLACEMENT, bands),
	          "ocean displacement spectrum");
	push.mod_factor[0] = TwoPi / normal_world.x;
	push.mod_factor[1] = TwoPi / normal_world.y;
	push.N[0] = push.N[1] = n;
	cmd.check(gr_ocean_generate_fft(cmd.get_context(), cmd.get_stream(), distribution_buffer_normal->get_device_pointer(),
	                                get_buffer(NormalInput)->get_device_pointer(), &push, GR_OCEAN_VARIANT_GRADIENT_NORMAL, bands),
	          "ocean normal spectrum");
}

void Ocean::compute_fft(HIP::CommandBuffer &cmd)
{
	auto &config = parameters.config;
	const unsigned n = config.fft_resolution, m = n >> config.displacement_downsample;
	auto run = [&](FFT &fft, unsigned input, unsigned output, unsigned size) {
		FFT::Resource src = {}, dst = {};
		HIP::Buffer *buffer = get_buffer(input);
		src.buffer.buffer = buffer;
		src.buffer.offset = 0;
		src.buffer.size = buffer->get_size();
		src.buffer.row_stride = size; // the C2R plan reads columns 0 .. N / 2 of the full spectrum
		src.buffer.layer_stride = size * size;
		dst.image.view = get_image(output); // level 0
		fft.execute(cmd, dst, src);
	};
	// One after the other on this stream: a plan is in flight on one stream at a time.
	run(displacement_fft, DisplacementInput, DisplacementOutput, m);
	run(height_fft, HeightInput, HeightOutput, n);
	run(normal_fft, NormalInput, NormalOutput, n);
}

void Ocean::bake_maps(HIP::CommandBuffer &cmd)
{
	auto &config = parameters.config;
	const unsigned n = config.fft_resolution, m = n >> config.displacement_downsample;
	gr_push_ocean_bake push = {};
	push.inv_size[0] = push.inv_size[1] = 1.0f / float(n);
	push.inv_size[2] = push.inv_size[3] = 1.0f / float(m);
	const vec2 delta_heightmap = {config.ocean_size.x / float(config.grid_count) / float(config.grid_resolution),
	                              config.ocean_size.y / float(config.grid_count) / float(config.grid_resolution)};
	const float down = float(1u << config.displacement_downsample);
	push.scale[0] = 1.0f / delta_heightmap.x;
	push.scale[1] = 1.0f / delta_heightmap.y;
	push.scale[2] = 1.0f / (delta_heightmap.x * down);
	push.scale[3] = 1.0f / (delta_heightmap.y * down);

	const gr_image height = get_image(HeightOutput)->get_level_view(0), displacement = get_image(DisplacementOutput)->get_level_view(0);
	const gr_image fragment = get_image(GradientJacobian)->get_level_view(0);
	gr_image vertex = {};
	if (config.heightmap)
		vertex = get_image(HeightDisplacement)->get_level_view(0);
	cmd.check(gr_ocean_bake_maps(cmd.get_context(), cmd.get_stream(), &height, &displacement, &fragment, config.heightmap ? &vertex : nullptr, &push),
	          "ocean bake maps");
}

void Ocean::generate_mipmaps(HIP::CommandBuffer &cmd)
{
	HIP::Image &normal = *get_image(NormalOutput);
	HIP::Image &fragment = *get_image(GradientJacobian);
	HIP::Image *vertex = get_image(HeightDisplacement);
	const auto vertex_mip_views = vertex ? level_views(*vertex, get_levels(HeightDisplacement)) : std::vector<gr_image>();
	const auto fragment_mip_views = level_views(fragment, fragment.get_levels());
	const auto normal_mip_views = level_views(normal, normal.get_levels());

	auto supports = [&](VkFormat format) { return !force_mipmap_shader && supports_single_pass_downsample(cmd.get_device(), format); };
	const bool support_spd_vert = !vertex_mip_views.empty() && supports(VkFormat(vertex_mip_views.front().format));
	const bool support_spd_frag = supports(VkFormat(fragment_mip_views.front().format));
	const bool support_spd_normal = supports(VkFormat(normal_mip_views.front().format));

	auto num_passes = unsigned(std::max(std::max(vertex_mip_views.size(), fragment_mip_views.size()), normal_mip_views.size()));
	if (support_spd_vert && support_spd_frag && support_spd_normal)
		num_passes = 2;

	auto single_pass = [&](const std::vector<gr_image> &views, bool zero_last_height, unsigned counter_slot) {
		const gr_image *output_mips[MaxSPDMips];
		vec4 filter_mods[MaxSPDMips];
		const unsigned num_mips = unsigned(views.size()) - 1;
		if (num_mips > MaxSPDMips)
			throw std::logic_error("Ocean: too many mip levels for the single-pass downsampler.");
		for (unsigned j = 0; j < num_mips; j++)
		{
			output_mips[j] = &views[j + 1];
			// The last heightmap level goes towards 0, so that padding edges transition cleanly.
			filter_mods[j] = zero_last_height && j + 1 == num_mips ? vec4(0.0f, 1.0f, 1.0f, 1.0f) : vec4(1.0f);
		}
		SPDInfo info = {};
		info.input = &views.front();
		info.output_mips = output_mips;
		info.num_mips = num_mips;
		info.counter_buffer = get_buffer(SpdCounter);
		info.counter_buffer_offset = 4 * counter_slot;
		info.num_components = 3;
		info.filter_mod = zero_last_height ? filter_mods : nullptr;
		emit_single_pass_downsample(cmd, info);
	};
	auto level = [&](const std::vector<gr_image> &views, unsigned i, const vec4 &filter_mod) {
		gr_push_ocean_mipmap push = {};
		push.result_mod[0] = filter_mod.x;
		push.result_mod[1] = filter_mod.y;
		push.result_mod[2] = filter_mod.z;
		push.result_mod[3] = filter_mod.w;
		push.inv_resolution[0] = 1.0f / float(views[i - 1].width);
		push.inv_resolution[1] = 1.0f / float(views[i - 1].height);
		push.count[0] = views[i].width;
		push.count[1] = views[i].height;
		push.lod = float(i - 1);
		cmd.check(gr_ocean_mipmap(cmd.get_context(), cmd.get_stream(), &views[i - 1], &views[i], &push), "ocean mipmap");
	};

	for (unsigned i = 1; i < num_passes; i++)
	{
		if (i == 1 && support_spd_vert)
		{
			if (vertex_mip_views.size() > 1)
				single_pass(vertex_mip_views, true, 0);
		}
		else if (!support_spd_vert && i < vertex_mip_views.size())
			level(vertex_mip_views, i, i + 1 == vertex_mip_views.size() ? vec4(0.0f, 1.0f, 1.0f, 1.0f) : vec4(1.0f));

		if (i == 1 && support_spd_frag)
			single_pass(fragment_mip_views, false, 1);
		else if (!support_spd_frag && i < fragment_mip_views.size())
			level(fragment_mip_views, i, vec4(1.0f));

		// RG16F has no single-pass downsampler here, so this chain is always level by level.
		if (!support_spd_normal && i < normal_mip_views.size())
			level(normal_mip_views, i, vec4(1.0f));
	}
}

void Ocean::update_fft_pass(HIP::CommandBuffer &cmd)
{
	if (!device || !distribution_buffer)
		throw std::logic_error("Ocean: update_fft_pass before on_device_created.");
	update_fft_input(cmd);
	compute_fft(cmd);
	bake_maps(cmd);
	generate_mipmaps(cmd);
}

void Ocean::build_lod_map(HIP::CommandBuffer &cmd)
{
	const gr_image image = get_image(Lods)->get_level_view(0);
	const gr_push_ocean_update_lod push = lod.update_lod_push();
	cmd.check(gr_ocean_update_lod(cmd.get_context(), cmd.get_stream(), &image, &push), "ocean update lod");
}

void Ocean::init_counter_buffer(HIP::CommandBuffer &cmd)
{
	HIP::Buffer *buffer = get_buffer(LodCounter);
	const gr_ocean_buffer counters = {buffer->get_device_pointer(), buffer->get_size()};
	uint32_t vertex_counts[16];
	lod.get_counts(vertex_counts);
	cmd.check(gr_ocean_init_counter_buffer(cmd.get_context(), cmd.get_stream(), &counters, vertex_counts), "ocean init counter buffer");
}

void Ocean::cull_blocks(HIP::CommandBuffer &cmd)
{
	const gr_image image = get_image(Lods)->get_level_view(0);
	HIP::Buffer *lod_buffer = get_buffer(LodData), *lod_counter_buffer = get_buffer(LodCounter);
	const gr_ocean_buffer patches = {lod_buffer->get_device_pointer(), lod_buffer->get_size()};
	const gr_ocean_buffer counters = {lod_counter_buffer->get_device_pointer(), lod_counter_buffer->get_size()};
	const gr_push_ocean_cull push = lod.cull_push();
	cmd.check(gr_ocean_cull_blocks(cmd.get_context(), cmd.get_stream(), &image, lod.get_wrap(), &patches, &counters, &push, lod.get_frustum()),
	          "ocean cull blocks");
}

// Three launches in stream order; the order stands in for the reference's barrier between the first two and the cull.
void Ocean::update_lod_pass(HIP::CommandBuffer &cmd)
{
	if (!device || !lod_request.lod_update)
		throw std::logic_error("Ocean: update_lod_pass before on_device_created, or on an ocean created without a LOD request.");
	build_lod_map(cmd);
	init_counter_buffer(cmd);
	cull_blocks(cmd);
}
} // namespace Granite
