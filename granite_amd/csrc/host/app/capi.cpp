// extern "C" surface of the harness (include/granite_app.h).  Exceptions from the C++ layer stop here.
#include "image_space_app.hpp"
#include "../timeline_trace.hpp"
#include "../post/ssr.hpp"
#include "../post/spd.hpp"
#include "../gtx.hpp"
#include "../texture_decoder.hpp"
#include "../texture_compression.hpp"
#include "../utils/image_utils.hpp"
#include "../fft/fft.hpp"
#include "../ocean.hpp"
#include "../post/hdr.hpp"
#include "../mesh/meshlet.hpp"
#include <cstdio>
#include <cstring>

using namespace Granite;

struct gra_app
{
	std::unique_ptr<ImageSpaceApplication> app;
	std::string error;
};

// Declared before the graph so that the graph, whose pass callback points at the ocean, goes first.
struct gra_ocean
{
	gra_app *app = nullptr;
	std::unique_ptr<Ocean> ocean;
	HIP::ImageHandle swapchain;
	std::unique_ptr<RenderGraph> graph;
	bool updated = false;
};

template <typename Fn>
static int guarded(gra_app *app, Fn &&fn)
{
	if (!app)
		return -1;
	try
	{
		fn();
		return 0;
	}
	catch (const std::exception &e)
	{
		app->error = e.what();
		return -1;
	}
}

template <typename Fn>
static int ocean_guarded(gra_ocean *ocean, Fn &&fn)
{
	if (!ocean)
		return -1;
	return guarded(ocean->app, fn);
}

static void unpack_mat4(mat4 &m, const float *src)
{
	memcpy(m.data(), src, 16 * sizeof(float));
}

template <typename Fn>
static int guarded_message(char *error, size_t error_size, Fn &&fn)
{
	try
	{
		fn();
		return 0;
	}
	catch (const std::exception &e)
	{
		if (error && error_size)
			snprintf(error, error_size, "%s", e.what());
		return -1;
	}
}

static void fill_gtx_info(gra_gtx_info *info, const GtxImage &img)
{
	info->type = img.type;
	info->format = uint32_t(img.format);
	info->width = img.width;
	info->height = img.height;
	info->depth = img.depth;
	info->layers = img.layers;
	info->levels = img.levels;
	info->flags = img.flags;
	info->payload_size = img.payload.size();
}

// A MESHLET4 file in 4-byte aligned memory and the view over it; throws with create_mesh_view's reason.
struct meshlet_file
{
	std::vector<uint32_t> words;
	Meshlet::MeshView view = {};
	explicit meshlet_file(const char *path)
	{
		FILE *f = fopen(path, "rb");
		if (!f)
			throw std::runtime_error(std::string("cannot open ") + path);
		fseek(f, 0, SEEK_END);
		const long size = ftell(f);
		fseek(f, 0, SEEK_SET);
		words.resize((size_t(size > 0 ? size : 0) + 3) / 4);
		const bool ok = size >= 0 && fread(words.data(), 1, size_t(size), f) == size_t(size);
		fclose(f);
		if (!ok)
			throw std::runtime_error(std::string("cannot read ") + path);
		std::string why;
		view = Meshlet::create_mesh_view(words.data(), size_t(size), &why);
		if (!view.format_header)
			throw std::runtime_error(std::string(path) + ": " + why);
	}
	void describe(gra_meshlet_info *info) const
	{
		*info = {};
		info->style = uint32_t(view.format_header->style);
		info->stream_count = view.format_header->stream_count;
		info->meshlet_count = view.format_header->meshlet_count;
		info->payload_size_words = view.format_header->payload_size_words;
		info->total_primitives = view.total_primitives;
		info->total_vertices = view.total_vertices;
		info->chunk_count = view.num_bounds_256;
	}
};

extern "C" {

gra_app *gra_create(const gra_config *config, char *error, size_t error_size)
{
	return gra_create_ext(config, nullptr, error, error_size);
}

gra_app *gra_create_ext(const gra_config *config, const gra_config_ext *ext, char *error, size_t error_size)
{
	try
	{
		if (!config)
			throw std::logic_error("null config");
		gra_config_ext settings = {};
		if (ext)
		{
			if (ext->struct_size < sizeof(uint32_t))
				throw std::logic_error("gra_config_ext.struct_size is smaller than the member itself.");
			memcpy(&settings, ext, ext->struct_size < sizeof(settings) ? ext->struct_size : sizeof(settings));
		}
		auto *handle = new gra_app;
		handle->app = std::make_unique<ImageSpaceApplication>(*config, settings);
		return handle;
	}
	catch (const std::exception &e)
	{
		if (error && error_size)
			snprintf(error, error_size, "%s", e.what());
		return nullptr;
	}
}

void gra_destroy(gra_app *app)
{
	delete app;
	Granite::TimelineTrace::get().flush(); // GRANITE_TIMELINE_TRACE: what the threads recorded goes to the file
}

const char *gra_last_error(gra_app *app)
{
	return app ? app->error.c_str() : "null app";
}

int gra_set_camera(gra_app *app, const float *projection16, const float *view16)
{
	return guarded(app, [&]() {
		mat4 p, v;
		unpack_mat4(p, projection16);
		unpack_mat4(v, view16);
		app->app->set_base_camera(p, v);
	});
}

int gra_set_camera_motion(gra_app *app, const float translation[3])
{
	return guarded(app, [&]() {
		if (!translation)
			throw std::logic_error("gra_set_camera_motion: null translation");
		app->app->set_camera_motion(vec3(translation[0], translation[1], translation[2]));
	});
}

int gra_set_render_parameters(gra_app *app, const float *f)
{
	return guarded(app, [&]() {
		RenderParameters rp = app->app->get_context().get_render_parameters();
		unpack_mat4(rp.projection, f);
		unpack_mat4(rp.view, f + 16);
		unpack_mat4(rp.view_projection, f + 32);
		unpack_mat4(rp.inv_projection, f + 48);
		unpack_mat4(rp.inv_view, f + 64);
		unpack_mat4(rp.inv_view_projection, f + 80);
		rp.unjittered_view_projection = rp.view_projection;
		rp.unjittered_inv_view_projection = rp.inv_view_projection;
		rp.camera_position = vec3(f[96], f[97], f[98]);
		rp.camera_front = vec3(f[99], f[100], f[101]);
		rp.z_near = f[102];
		rp.z_far = f[103];
		app->app->get_context().set_render_parameters(rp);
	});
}

int gra_get_render_parameters(gra_app *app, float *f)
{
	return guarded(app, [&]() {
		auto &rp = app->app->get_context().get_render_parameters();
		const mat4 *mats[6] = {&rp.projection, &rp.view, &rp.view_projection, &rp.inv_projection, &rp.inv_view, &rp.inv_view_projection};
		for (int i = 0; i < 6; i++)
			memcpy(f + 16 * i, mats[i]->data(), 16 * sizeof(float));
		for (int i = 0; i < 3; i++)
		{
			f[96 + i] = rp.camera_position[i];
			f[99 + i] = rp.camera_front[i];
		}
		f[102] = rp.z_near;
		f[103] = rp.z_far;
	});
}

int gra_set_lights(gra_app *app, const gra_light_desc *lights, uint32_t count)
{
	return guarded(app, [&]() { app->app->set_lights(lights, count); });
}

int gra_set_decal_texture(gra_app *app, uint32_t index, uint32_t width, uint32_t height, uint32_t levels, uint32_t format, const void *texels)
{
	return guarded(app, [&]() { app->app->set_decal_texture(index, width, height, levels, format, texels); });
}

int gra_set_decals(gra_app *app, const gra_decal_desc *decals, uint32_t count)
{
	return guarded(app, [&]() { app->app->set_decals(decals, count); });
}

int gra_get_sky_state(gra_app *app, float local_view_projection16[16], float inv_local_view_projection16[16], float color[3], float *camera_height,
                      float direction[3])
{
	return guarded(app, [&]() {
		const RenderContext &context = app->app->get_context();
		const auto &rp = context.get_render_parameters();
		if (local_view_projection16)
			memcpy(local_view_projection16, rp.local_view_projection.data(), 16 * sizeof(float));
		if (inv_local_view_projection16)
			memcpy(inv_local_view_projection16, rp.inv_local_view_projection.data(), 16 * sizeof(float));
		const Skybox::RenderInfo info = app->app->get_skybox().get_render_info(context);
		for (int i = 0; i < 3; i++)
		{
			if (color)
				color[i] = info.color[i];
			if (direction)
				direction[i] = info.direction[i];
		}
		if (camera_height)
			*camera_height = info.camera_height;
	});
}

int gra_set_sky_cube(gra_app *app, uint32_t size, uint32_t levels, const void *rgba16f_chain, const float color[3])
{
	return guarded(app, [&]() { app->app->set_sky_cube(size, levels, rgba16f_chain, color); });
}

int gra_set_sky_cube_gtx(gra_app *app, const char *cube_gtx, const float color[3])
{
	return guarded(app, [&]() {
		if (!cube_gtx)
			throw std::logic_error("gra_set_sky_cube_gtx: null path");
		const GtxImage image = gtx_load(cube_gtx);
		if (image.format != VK_FORMAT_R16G16B16A16_SFLOAT || image.layers != 6 || image.depth != 1 || image.width != image.height)
			throw std::logic_error(std::string("gra_set_sky_cube_gtx: ") + cube_gtx + " is not a square R16G16B16A16_SFLOAT image of 6 layers (a cube as gra_environment_bake writes it).");
		app->app->set_sky_cube(image.width, image.levels, image.payload.data(), color);
	});
}

int gra_get_decal_state(gra_app *app, uint32_t *count, uint32_t *order, float *world_to_texture, float *mvps, uint32_t *ranges)
{
	return guarded(app, [&]() {
		auto &cluster = app->app->get_clusterer();
		const auto &sorted = cluster.get_decal_order();
		if (!count)
			throw std::logic_error("gra_get_decal_state: null count");
		*count = uint32_t(sorted.size());
		if (order)
			memcpy(order, sorted.data(), sorted.size() * sizeof(uint32_t));
		if (world_to_texture)
			memcpy(world_to_texture, cluster.get_packed_decal_transforms().data(), sorted.size() * sizeof(mat_affine));
		if (mvps)
			memcpy(mvps, cluster.get_packed_decal_mvps().data(), sorted.size() * sizeof(mat4));
		if (ranges)
			memcpy(ranges, cluster.get_decal_index_range().data(), sorted.size() * sizeof(uvec2));
	});
}

int gra_upload_gbuffer(gra_app *app, const void *emissive, const void *albedo, const void *normal, const void *pbr, const void *depth,
                       const void *mv)
{
	return guarded(app, [&]() { app->app->upload_gbuffer(emissive, albedo, normal, pbr, depth, mv); });
}

int gra_compute_rec709_to_display(const float *primaries8, float *out9)
{
	if (!primaries8 || !out9)
		return -1;
	HdrMetadata md;
	memcpy(md.display_primary_red, primaries8, 8);
	memcpy(md.display_primary_green, primaries8 + 2, 8);
	memcpy(md.display_primary_blue, primaries8 + 4, 8);
	memcpy(md.white_point, primaries8 + 6, 8);
	compute_rec709_to_st2020(md, out9);
	return 0;
}

int gra_gtx_probe(const char *path, gra_gtx_info *info, char *error, size_t error_size)
{
	return guarded_message(error, error_size, [&]() {
		if (!path || !info)
			throw std::logic_error("gra_gtx_probe: null argument");
		fill_gtx_info(info, gtx_load(path));
	});
}

int gra_gtx_read(const char *path, void *payload, uint64_t payload_capacity, char *error, size_t error_size)
{
	return guarded_message(error, error_size, [&]() {
		if (!path || !payload)
			throw std::logic_error("gra_gtx_read: null argument");
		auto img = gtx_load(path);
		if (img.payload.size() > payload_capacity)
			throw std::logic_error("gra_gtx_read: destination is smaller than the payload");
		memcpy(payload, img.payload.data(), img.payload.size());
	});
}

int gra_gtx_write(const char *path, const gra_gtx_info *info, const void *payload, char *error, size_t error_size)
{
	return guarded_message(error, error_size, [&]() {
		if (!path || !info || !payload)
			throw std::logic_error("gra_gtx_write: null argument");
		GtxImage img;
		img.type = info->type;
		img.format = VkFormat(info->format);
		img.width = info->width;
		img.height = info->height;
		img.depth = info->depth;
		img.layers = info->layers;
		img.levels = info->levels;
		img.flags = info->flags;
		if (info->payload_size != img.required_payload_size())
			throw std::logic_error("gra_gtx_write: payload_size does not match the layout of the described image");
		img.payload.assign(static_cast<const uint8_t *>(payload), static_cast<const uint8_t *>(payload) + info->payload_size);
		gtx_save(img, path);
	});
}

int gra_gtx_decode(gra_app *app, const char *src_path, const char *dst_path)
{
	return guarded(app, [&]() {
		if (!src_path || !dst_path)
			throw std::logic_error("gra_gtx_decode: null path");
		auto &device = app->app->get_device();
		if (!device.get_context())
			throw std::logic_error("gra_gtx_decode: the application has no device");
		gtx_save(decode_compressed_image(device.get_context(), nullptr, gtx_load(src_path)), dst_path);
	});
}

int gra_gtx_encode(gra_app *app, const char *src_path, const char *dst_path, uint32_t format, int generate_mipmaps_)
{
	return guarded(app, [&]() {
		if (!src_path || !dst_path)
			throw std::logic_error("gra_gtx_encode: null path");
		auto &device = app->app->get_device();
		if (!device.get_context())
			throw std::logic_error("gra_gtx_encode: the application has no device");
		GtxImage image = gtx_load(src_path);
		if (generate_mipmaps_)
			image = generate_mipmaps(device.get_context(), nullptr, image);
		CompressorArguments args;
		args.format = VkFormat(format);
		gtx_save(compress_texture(device.get_context(), nullptr, args, image), dst_path);
	});
}

uint32_t gra_string_to_format(const char *name)
{
	return name ? uint32_t(string_to_format(name)) : 0u;
}

int gra_gtx_encode_layout(const gra_gtx_info *input, uint32_t format, int generate_mipmaps_, gra_gtx_info *output, uint64_t *level_offsets,
                          uint32_t level_capacity, char *error, size_t error_size)
{
	return guarded_message(error, error_size, [&]() {
		if (!input || !output)
			throw std::logic_error("gra_gtx_encode_layout: null argument");
		GtxImage img;
		img.type = input->type;
		img.format = VkFormat(input->format);
		img.width = input->width;
		img.height = input->height;
		img.depth = input->depth;
		img.layers = input->layers;
		img.levels = input->levels;
		img.flags = input->flags;
		if (!img.width || !img.height || img.depth != 1 || !img.layers || !img.levels || img.levels > 16 || img.width > 65536u || img.height > 65536u ||
		    img.layers > 65536u)
			throw std::logic_error("gra_gtx_encode_layout: empty, 3-D or implausible dimensions");
		if (!vk_format_payload_block_size(VkFormat(format)))
			throw std::logic_error("gra_gtx_encode_layout: format " + std::to_string(format) + " is not one the executor handles");
		if (generate_mipmaps_)
		{
			img.levels = num_miplevels(img.width, img.height);
			img.flags &= ~2u;
		}
		const GtxImage out = compressed_layout(img, VkFormat(format));
		fill_gtx_info(output, out);
		for (uint32_t l = 0; level_offsets && l < level_capacity && l < out.levels; l++)
			level_offsets[l] = out.level_offset(l);
	});
}

int gra_environment_bake(gra_app *app, const char *equirect_gtx, float cube_scale, const char *cube_path, const char *reflection_path,
                         const char *irradiance_path)
{
	return guarded(app, [&]() {
		if (!equirect_gtx)
			throw std::logic_error("gra_environment_bake: null input path");
		auto &device = app->app->get_device();
		if (!device.get_context())
			throw std::logic_error("gra_environment_bake: the application has no device");
		gr_ctx *ctx = device.get_context();
		const GtxImage cube = convert_equirect_to_cube(ctx, nullptr, gtx_load(equirect_gtx), cube_scale);
		if (cube_path)
			gtx_save(cube, cube_path);
		if (reflection_path)
			gtx_save(convert_cube_to_ibl_specular(ctx, nullptr, cube), reflection_path);
		if (irradiance_path)
			gtx_save(convert_cube_to_ibl_diffuse(ctx, nullptr, cube), irradiance_path);
	});
}

void gra_ocean_default_config(gra_ocean_config *config)
{
	if (!config)
		return;
	const OceanConfig defaults;
	*config = {};
	config->fft_resolution = defaults.fft_resolution;
	config->displacement_downsample = defaults.displacement_downsample;
	config->grid_count = defaults.grid_count;
	config->grid_resolution = defaults.grid_resolution;
	config->ocean_size[0] = defaults.ocean_size.x;
	config->ocean_size[1] = defaults.ocean_size.y;
	config->wind_velocity[0] = defaults.wind_velocity.x;
	config->wind_velocity[1] = defaults.wind_velocity.y;
	config->normal_mod = defaults.normal_mod;
	config->amplitude = defaults.amplitude;
	config->heightmap = defaults.heightmap ? 1u : 0u;
	config->lod_bias = defaults.lod_bias;
	for (float &band : config->frequency_bands)
		band = 1.0f;
}

int gra_ocean_create(gra_app *app, const gra_ocean_config *config, gra_ocean **ocean)
{
	return guarded(app, [&]() {
		if (!config || !ocean)
			throw std::logic_error("gra_ocean_create: null config or result");
		*ocean = nullptr;
		OceanConfig c;
		c.fft_resolution = config->fft_resolution;
		c.displacement_downsample = config->displacement_downsample;
		c.grid_count = config->grid_count;
		c.grid_resolution = config->grid_resolution;
		c.ocean_size = vec2(config->ocean_size[0], config->ocean_size[1]);
		c.wind_velocity = vec2(config->wind_velocity[0], config->wind_velocity[1]);
		c.normal_mod = config->normal_mod;
		c.amplitude = config->amplitude;
		c.heightmap = config->heightmap != 0;
		c.lod_bias = config->lod_bias;
		auto handle = std::make_unique<gra_ocean>();
		handle->app = app;
		OceanLodRequest lod;
		lod.lod_update = config->lod_update != 0;
		lod.fixed_position = config->fixed_position != 0;
		lod.center_position = vec3(config->center_position[0], config->center_position[1], config->center_position[2]);
		handle->ocean = std::make_unique<Ocean>(c, config->force_mipmap_shader != 0, lod); // refuses before anything is allocated
		auto &device = app->app->get_device();
		if (!device.get_context())
			throw std::logic_error("gra_ocean_create: the application has no device");
		device.wait_idle();
		handle->ocean->set_frequency_band_modulation(config->freq_band_modulation != 0);
		for (unsigned i = 0; i < Ocean::FrequencyBands; i++)
			handle->ocean->set_frequency_band_amplitude(i, config->frequency_bands[i]);
		handle->ocean->on_device_created(device);
		if (config->through_render_graph)
		{
			// A graph of the ocean's own: the update pass, and a pass that consumes everything it writes and produces the backbuffer,
			// so that nothing of the update is culled or aliased before it is read back.
			const unsigned n = c.fft_resolution;
			handle->graph = std::make_unique<RenderGraph>();
			auto &graph = *handle->graph;
			graph.set_device(&device);
			ResourceDimensions dim;
			dim.width = n;
			dim.height = n;
			dim.format = VK_FORMAT_R16G16B16A16_SFLOAT;
			graph.set_backbuffer_dimensions(dim);
			if (lod.lod_update)
				handle->ocean->add_lod_update_pass(graph); // before the FFT update, as add_render_passes has them
			handle->ocean->add_fft_update_pass(graph);
			auto &present = graph.add_pass("ocean-present", RENDER_GRAPH_QUEUE_COMPUTE_BIT);
			if (lod.lod_update)
			{
				present.add_texture_input(Ocean::ResourceNames[GRA_OCEAN_LODS]);
				present.add_storage_read_only_input(Ocean::ResourceNames[GRA_OCEAN_LOD_COUNTER]);
				present.add_storage_read_only_input(Ocean::ResourceNames[GRA_OCEAN_LOD_DATA]);
			}
			for (unsigned i = 0; i < Ocean::ResourceCount; i++)
			{
				if (i <= GRA_OCEAN_DISPLACEMENT_FFT_INPUT || i == GRA_OCEAN_SPD_COUNTER)
					present.add_storage_read_only_input(Ocean::ResourceNames[i]);
				else if (i != GRA_OCEAN_HEIGHT_DISPLACEMENT_OUTPUT || c.heightmap)
					present.add_texture_input(Ocean::ResourceNames[i]);
			}
			AttachmentInfo out;
			out.size_class = SizeClass::Absolute;
			out.size_x = out.size_y = float(n);
			out.format = VK_FORMAT_R16G16B16A16_SFLOAT;
			auto *target = &present.add_storage_texture_output("ocean-present-output", out);
			RenderGraph *g = handle->graph.get();
			present.set_build_render_pass([g, target](HIP::CommandBuffer &cmd) { cmd.clear_image(g->get_physical_texture_resource(*target)); });
			graph.set_backbuffer_source("ocean-present-output");
			graph.bake();
			handle->swapchain = device.create_image(n, n, VK_FORMAT_R16G16B16A16_SFLOAT, "ocean-present-swapchain");
		}
		else
			handle->ocean->create_resources(device);
		*ocean = handle.release();
	});
}

int gra_ocean_update(gra_ocean *ocean, double elapsed_time)
{
	return ocean_guarded(ocean, [&]() {
		auto &device = ocean->app->app->get_device();
		ocean->ocean->set_elapsed_time(elapsed_time);
		if (ocean->graph)
		{
			TaskComposer composer;
			ocean->graph->setup_attachments(device, ocean->swapchain.get());
			ocean->graph->enqueue_render_passes(device, composer);
		}
		else
		{
			HIP::CommandBuffer cmd(device, device.get_stream(HIP::CommandBuffer::Type::Generic), HIP::CommandBuffer::Type::Generic);
			if (ocean->ocean->has_lod_update())
				ocean->ocean->update_lod_pass(cmd);
			ocean->ocean->update_fft_pass(cmd);
		}
		device.wait_idle();
		ocean->updated = true;
	});
}

int gra_ocean_describe(gra_ocean *ocean, uint32_t which, gra_ocean_resource_info *info)
{
	return ocean_guarded(ocean, [&]() {
		if (!info || which >= Ocean::TotalResourceCount)
			throw std::logic_error("gra_ocean_describe: null info or unknown resource");
		if (ocean->graph && !ocean->updated)
			throw std::logic_error("gra_ocean_describe: a graph's resources exist after the first update");
		*info = {};
		if (HIP::Buffer *buffer = ocean->ocean->get_buffer(which))
		{
			info->exists = 1;
			info->size_bytes = buffer->get_size();
		}
		else if (HIP::Image *image = ocean->ocean->get_image(which))
		{
			info->exists = info->is_image = 1;
			info->width = image->get_width();
			info->height = image->get_height();
			info->format = uint32_t(image->get_format());
			info->levels = ocean->ocean->get_levels(which);
			const gr_image view = image->get_level_view(0);
			info->size_bytes = uint64_t(view.pitch_bytes) * view.height;
		}
	});
}

int gra_ocean_read(gra_ocean *ocean, uint32_t which, uint32_t level, void *out, uint64_t size)
{
	return ocean_guarded(ocean, [&]() {
		if (!out || which >= Ocean::TotalResourceCount)
			throw std::logic_error("gra_ocean_read: null output or unknown resource");
		if (!ocean->updated)
			throw std::logic_error("gra_ocean_read: nothing has been computed yet");
		auto &device = ocean->app->app->get_device();
		gr_ctx *ctx = device.get_context();
		const void *src = nullptr;
		uint64_t bytes = 0;
		if (HIP::Buffer *buffer = ocean->ocean->get_buffer(which))
		{
			if (level != 0)
				throw std::logic_error("gra_ocean_read: a buffer has one level");
			src = buffer->get_device_pointer();
			bytes = buffer->get_size();
		}
		else if (HIP::Image *image = ocean->ocean->get_image(which))
		{
			if (level >= ocean->ocean->get_levels(which))
				throw std::logic_error("gra_ocean_read: the resource has no such level");
			const gr_image view = image->get_level_view(level);
			src = view.ptr;
			bytes = uint64_t(view.pitch_bytes) * view.height;
		}
		else
			throw std::logic_error(std::string("gra_ocean_read: ") + Ocean::ResourceNames[which] + " does not exist");
		if (size != bytes)
			throw std::logic_error("gra_ocean_read: size is not that of the level");
		if (gr_download(ctx, nullptr, out, src, size_t(bytes)) < 0 || gr_sync(ctx, nullptr) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	});
}

int gra_ocean_distribution(gra_ocean *ocean, uint32_t which, void *out)
{
	return ocean_guarded(ocean, [&]() {
		auto &d = ocean->ocean->get_distributions();
		const std::vector<vec2> *source = which == GRA_OCEAN_DISTRIBUTION_HEIGHT         ? &d.height
		                                  : which == GRA_OCEAN_DISTRIBUTION_DISPLACEMENT ? &d.displacement
		                                  : which == GRA_OCEAN_DISTRIBUTION_NORMAL       ? &d.normal
		                                                                                 : nullptr;
		if (!out || !source)
			throw std::logic_error("gra_ocean_distribution: null output or unknown distribution");
		memcpy(out, source->data(), source->size() * sizeof(vec2));
	});
}

int gra_ocean_parameters(gra_ocean *ocean, float *out8)
{
	return ocean_guarded(ocean, [&]() {
		if (!out8)
			throw std::logic_error("gra_ocean_parameters: null output");
		const vec2 world = ocean->ocean->heightmap_world_size(), normal = ocean->ocean->normalmap_world_size(), wind = ocean->ocean->get_wind_direction();
		const float values[8] = {world.x, world.y, normal.x, normal.y, wind.x, wind.y, ocean->ocean->get_phillips_L(), ocean->ocean->get_config().amplitude};
		memcpy(out8, values, sizeof(values));
	});
}

int gra_ocean_set_camera(gra_ocean *ocean, const float position[3], const float planes[24])
{
	return ocean_guarded(ocean, [&]() {
		if (!position || !planes)
			throw std::logic_error("gra_ocean_set_camera: null position or planes");
		vec4 p[6];
		for (unsigned i = 0; i < 6; i++)
			p[i] = vec4(planes[4 * i], planes[4 * i + 1], planes[4 * i + 2], planes[4 * i + 3]);
		ocean->ocean->set_camera(vec3(position[0], position[1], position[2]), p);
	});
}

int gra_ocean_draw_info(gra_ocean *ocean, struct gra_ocean_draw_info *out)
{
	return ocean_guarded(ocean, [&]() {
		if (!out)
			throw std::logic_error("gra_ocean_draw_info: null output");
		const OceanDrawInfo info = ocean->ocean->get_lod().get_draw_info();
		static_assert(sizeof(out->data) == sizeof(info.data), "gra_ocean_draw_info carries OceanData");
		memcpy(out->data, &info.data, sizeof(out->data));
		out->lods = info.lods;
		out->lod_stride = info.lod_stride;
		out->border_count = info.border_count;
		out->index_type = info.index_type;
	});
}

// The mesh `which` names: host copies, and the device buffers where the ocean made them.
struct ocean_mesh
{
	const void *vertices = nullptr, *indices = nullptr;
	uint32_t vertex_count = 0, vertex_stride = 0, index_count = 0;
	HIP::Buffer *vbo = nullptr, *ibo = nullptr;
};
static ocean_mesh find_ocean_mesh(gra_ocean *ocean, uint32_t which)
{
	ocean_mesh m;
	const OceanLod &lod = ocean->ocean->get_lod();
	if (which == GRA_OCEAN_MESH_BORDER)
	{
		const OceanBorderMesh &border = lod.get_border_mesh();
		m = {border.positions.data(), border.indices.data(), uint32_t(border.positions.size()), uint32_t(sizeof(vec3)), uint32_t(border.indices.size()),
		     ocean->ocean->get_border_vbo(), ocean->ocean->get_border_ibo()};
	}
	else if (which < lod.get_lod_count())
	{
		const OceanLodMesh &mesh = lod.get_lod_mesh(which);
		m = {mesh.vertices.data(), mesh.indices.data(), uint32_t(mesh.vertices.size()), uint32_t(sizeof(OceanVertex)), uint32_t(mesh.indices.size()),
		     ocean->ocean->get_lod_vbo(which), ocean->ocean->get_lod_ibo(which)};
	}
	return m;
}

int gra_ocean_mesh_describe(gra_ocean *ocean, uint32_t which, gra_ocean_mesh_info *info)
{
	return ocean_guarded(ocean, [&]() {
		if (!info)
			throw std::logic_error("gra_ocean_mesh_describe: null info");
		const ocean_mesh m = find_ocean_mesh(ocean, which);
		*info = {};
		info->exists = m.vertex_count != 0 ? 1u : 0u;
		info->on_device = m.vbo && m.ibo ? 1u : 0u;
		info->vertex_count = m.vertex_count;
		info->vertex_stride = m.vertex_stride;
		info->index_count = m.index_count;
		info->index_stride = uint32_t(sizeof(uint16_t));
	});
}

int gra_ocean_mesh_read(gra_ocean *ocean, uint32_t which, void *vbo_out, void *ibo_out)
{
	return ocean_guarded(ocean, [&]() {
		const ocean_mesh m = find_ocean_mesh(ocean, which);
		if (!vbo_out || !ibo_out || m.vertex_count == 0)
			throw std::logic_error("gra_ocean_mesh_read: null output or a mesh that does not exist");
		const size_t vertex_bytes = size_t(m.vertex_count) * m.vertex_stride, index_bytes = size_t(m.index_count) * sizeof(uint16_t);
		if (m.vbo && m.ibo)
		{
			gr_ctx *ctx = ocean->app->app->get_device().get_context();
			if (m.vbo->get_size() != vertex_bytes || m.ibo->get_size() != index_bytes)
				throw std::logic_error("gra_ocean_mesh_read: a device buffer does not have its mesh's size");
			if (gr_download(ctx, nullptr, vbo_out, m.vbo->get_device_pointer(), vertex_bytes) < 0 ||
			    gr_download(ctx, nullptr, ibo_out, m.ibo->get_device_pointer(), index_bytes) < 0 || gr_sync(ctx, nullptr) < 0)
				throw std::runtime_error(gr_last_error(ctx));
		}
		else
		{
			memcpy(vbo_out, m.vertices, vertex_bytes);
			memcpy(ibo_out, m.indices, index_bytes);
		}
	});
}

void gra_ocean_destroy(gra_ocean *ocean)
{
	if (!ocean)
		return;
	ocean->app->app->get_device().wait_idle();
	delete ocean;
}

int gra_meshlet_describe(const char *path, gra_meshlet_info *info, char *error, size_t error_size)
{
	return guarded_message(error, error_size, [&]() {
		if (!path || !info)
			throw std::logic_error("gra_meshlet_describe: null argument");
		meshlet_file(path).describe(info);
	});
}

int gra_meshlet_decode(gra_app *app, const char *path, const gra_meshlet_request *request, gra_meshlet_info *result)
{
	return guarded(app, [&]() {
		if (!path || !request)
			throw std::logic_error("gra_meshlet_decode: null path or request");
		gr_ctx *ctx = app->app->get_device().get_context();
		if (!ctx)
			throw std::logic_error("gra_meshlet_decode: the application has no device");
		const meshlet_file file(path);
		const Meshlet::MeshView &view = file.view;
		if (request->target_style > uint32_t(view.format_header->style))
			throw std::logic_error("gra_meshlet_decode: target_style is above the file's style");
		if (request->runtime_style > 1u || (request->flags & ~(GR_MESHLET_DECODE_UNROLLED_MESH | GR_MESHLET_DECODE_INDEX_16)))
			throw std::logic_error("gra_meshlet_decode: unknown runtime_style or flags");
		const uint64_t index_bytes = (request->flags & GR_MESHLET_DECODE_UNROLLED_MESH) ? 4 : ((request->flags & GR_MESHLET_DECODE_INDEX_16) ? 2 : 1);
		const uint64_t primitives = uint64_t(request->primitive_offset) + view.total_primitives, vertices = uint64_t(request->vertex_offset) + view.total_vertices;
		const auto runtime_style = request->runtime_style ? Meshlet::RuntimeStyle::Meshlet : Meshlet::RuntimeStyle::MDI;
		struct Array
		{
			const char *name;
			void *host;
			uint64_t bytes, least;
			bool needed;
			void *device = nullptr;
		} arrays[5] = {{"indices", request->indices, request->indices_bytes, primitives * 3 * index_bytes, true},
		               {"positions", request->positions, request->positions_bytes, vertices * 12, true},
		               {"attributes", request->attributes, request->attributes_bytes, vertices * 16, request->target_style >= 1u},
		               {"skin", request->skin, request->skin_bytes, vertices * 8, request->target_style >= 2u},
		               {"indirect", request->indirect, request->indirect_bytes, view.num_bounds_256 * Meshlet::indirect_stride(runtime_style), false}};
		struct Release
		{
			gr_ctx *ctx;
			Array *arrays;
			~Release()
			{
				for (int i = 0; i < 5; i++)
					if (arrays[i].device)
						gr_free(ctx, arrays[i].device);
			}
		} release{ctx, arrays};
		auto check = [&](int code) {
			if (code < 0)
				throw std::runtime_error(gr_last_error(ctx));
		};
		for (Array &a : arrays)
		{
			if (!a.host && !a.needed)
				continue;
			if (a.bytes < a.least || (!a.host && a.bytes))
				throw std::logic_error(std::string("gra_meshlet_decode: ") + a.name + " is null or smaller than the decode needs");
			check(gr_alloc(ctx, a.bytes ? a.bytes : 16, &a.device)); // a mesh of empty meshlets still names its buffers
			if (a.bytes)
				check(gr_upload(ctx, nullptr, a.device, a.host, a.bytes));
		}
		Meshlet::DecodeInfo info;
		info.ibo = {arrays[0].device, arrays[0].bytes};
		for (int i = 0; i < 3; i++)
			info.streams[i] = {arrays[1 + i].device, arrays[1 + i].bytes};
		info.indirect = {arrays[4].device, arrays[4].bytes};
		info.flags = request->flags;
		info.target_style = Meshlet::MeshStyle(request->target_style);
		info.runtime_style = runtime_style;
		info.push.primitive_offset = request->primitive_offset;
		info.push.vertex_offset = request->vertex_offset;
		std::string why;
		if (view.format_header->meshlet_count && !Meshlet::decode_mesh(ctx, nullptr, info, view, &why))
			throw std::runtime_error(why);
		for (Array &a : arrays)
			if (a.device && a.bytes)
				check(gr_download(ctx, nullptr, a.host, a.device, a.bytes));
		check(gr_sync(ctx, nullptr));
		if (result)
			file.describe(result);
	});
}

int gra_fft_transform(gra_app *app, const gra_fft_request *request)
{
	return guarded(app, [&]() {
		if (!request || !request->input || !request->output || request->input_bytes == 0 || request->output_bytes == 0)
			throw std::logic_error("gra_fft_transform: null request, input or output");
		if (request->mode > GR_FFT_COMPLEX_TO_REAL || request->data_type > GR_FFT_FP16)
			throw std::logic_error("gra_fft_transform: unknown mode or data type");
		auto &device = app->app->get_device();
		gr_ctx *ctx = device.get_context();
		if (!ctx)
			throw std::logic_error("gra_fft_transform: the application has no device");
		const bool texture = request->image_width != 0;
		const bool fp16 = request->data_type == GR_FFT_FP16, real_out = request->mode == GR_FFT_COMPLEX_TO_REAL;
		const VkFormat format = real_out ? (fp16 ? VK_FORMAT_R16_SFLOAT : VK_FORMAT_R32_SFLOAT) : (fp16 ? VK_FORMAT_R16G16_SFLOAT : VK_FORMAT_R32G32_SFLOAT);
		if (texture)
		{
			const uint64_t image_bytes = uint64_t(request->image_width) * request->image_height * vk_format_block_size(format);
			if (request->image_height == 0 || request->image_byte_offset > request->output_bytes || image_bytes > request->output_bytes - request->image_byte_offset)
				throw std::logic_error("gra_fft_transform: the image does not lie inside the output block");
		}

		FFT::Options options;
		options.Nx = request->nx;
		options.Ny = request->ny;
		options.Nz = request->nz;
		options.dimensions = request->dimensions;
		options.mode = FFT::Mode(request->mode);
		options.data_type = FFT::DataType(request->data_type);
		options.output_resource = texture ? FFT::ResourceType::Texture : FFT::ResourceType::Buffer;
		FFT fft;
		if (!fft.plan(&device, options))
			throw std::runtime_error(std::string("gra_fft_transform: ") + gr_last_error(ctx));

		device.wait_idle();
		auto stream = device.get_stream(HIP::CommandBuffer::Type::Generic);
		auto input = device.create_buffer(request->input_bytes, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, "fft-input");
		auto output = device.create_buffer(request->output_bytes, VK_BUFFER_USAGE_STORAGE_BUFFER_BIT, "fft-output");
		if (gr_upload(ctx, stream, input->get_device_pointer(), request->input, request->input_bytes) < 0 ||
		    gr_upload(ctx, stream, output->get_device_pointer(), request->output, request->output_bytes) < 0)
			throw std::runtime_error(gr_last_error(ctx));

		FFT::Resource src = {}, dst = {};
		src.buffer = {input.get(), 0, size_t(request->input_bytes), request->input_row_stride, request->input_layer_stride};
		std::unique_ptr<HIP::Image> image;
		if (texture)
		{
			image.reset(new HIP::Image(request->image_width, request->image_height, format,
			                           static_cast<uint8_t *>(output->get_device_pointer()) + request->image_byte_offset));
			dst.image = {image.get(), {request->output_offset[0], request->output_offset[1]}};
		}
		else
			dst.buffer = {output.get(), 0, size_t(request->output_bytes), request->output_row_stride, request->output_layer_stride};
		HIP::CommandBuffer cmd(device, stream, HIP::CommandBuffer::Type::Generic);
		fft.execute(cmd, dst, src);
		if (gr_download(ctx, stream, request->output, output->get_device_pointer(), request->output_bytes) < 0 || gr_sync(ctx, stream) < 0)
			throw std::runtime_error(gr_last_error(ctx));
		fft.release();
	});
}

int gra_upload_aa_bench_images(gra_app *app, const void *rgba8_first, const void *rgba8_second, uint32_t width, uint32_t height)
{
	return guarded(app, [&]() { app->app->upload_aa_bench_images(rgba8_first, rgba8_second, width, height); });
}

int gra_upload_ambient_occlusion(gra_app *app, const void *ao_r8)
{
	return guarded(app, [&]() { app->app->upload_ambient_occlusion(ao_r8); });
}

int gra_upload_gbuffer_gtx(gra_app *app, const char *emissive, const char *albedo, const char *normal, const char *pbr,
                           const char *depth, const char *motion_vectors)
{
	return guarded(app, [&]() {
		const char *paths[6] = {emissive, albedo, normal, pbr, depth, motion_vectors};
		app->app->upload_gbuffer_gtx(paths);
	});
}

int gra_get_render_size(gra_app *app, uint32_t *width, uint32_t *height)
{
	return guarded(app, [&]() {
		if (!width || !height)
			throw std::logic_error("gra_get_render_size: null output");
		*width = app->app->get_render_width();
		*height = app->app->get_render_height();
	});
}

int gra_render_frames(gra_app *app, uint32_t count, int32_t sync)
{
	return guarded(app, [&]() {
		for (uint32_t i = 0; i < count; i++)
			app->app->render_frame();
		if (sync)
			app->app->wait_idle();
	});
}

int gra_set_exchange_callback(gra_app *app, gra_exchange_fn fn, void *user)
{
	return guarded(app, [&]() { app->app->set_exchange_callback(fn, user); });
}

int gra_comm_create_unique_id(uint8_t *id128)
{
	if (!id128)
		return -1;
	try
	{
		HIP::Collective::create_unique_id(id128);
		return 0;
	}
	catch (const std::exception &e)
	{
		fprintf(stderr, "gra_comm_create_unique_id: %s\n", e.what());
		return -1;
	}
}

int gra_comm_init(gra_app *app, const uint8_t *id128, int32_t rank, int32_t ranks)
{
	return guarded(app, [&]() {
		if (!id128)
			throw std::logic_error("gra_comm_init: null id");
		app->app->init_collective(id128, rank, ranks);
	});
}

int gra_comm_info(gra_app *app, int32_t *nranks, int32_t *version, int32_t *stand_in)
{
	return guarded(app, [&]() {
		auto &c = app->app->get_collective();
		if (!c.is_initialized())
			throw std::logic_error("gra_comm_info: no communicator (gra_comm_init)");
		if (nranks)
			*nranks = c.communicator_ranks();
		if (version)
			*version = HIP::Collective::library_version();
		if (stand_in)
			*stand_in = HIP::Collective::is_stand_in() ? 1 : 0;
	});
}

int gra_comm_init_output(gra_app *app, const uint8_t *id128, int32_t rank, int32_t ranks)
{
	return guarded(app, [&]() {
		if (!id128)
			throw std::logic_error("gra_comm_init_output: null id");
		app->app->init_output_collective(id128, rank, ranks);
	});
}

int gra_get_strip_plan(gra_app *app, uint32_t *out24)
{
	return guarded(app, [&]() {
		if (!out24)
			throw std::logic_error("gra_get_strip_plan: null output");
		auto &p = app->app->get_strip_plan();
		uint32_t *o = out24;
		*o++ = p.index; *o++ = p.count; *o++ = p.width; *o++ = p.height;
		for (const Granite::RowRange *r : {&p.lighting, &p.threshold, &p.d0, &p.d1, &p.u0, &p.tonemap})
		{
			*o++ = r->whole ? 1u : 0u;
			*o++ = r->first;
			*o++ = r->count;
		}
		*o++ = p.d1_chunk_rows;
		*o++ = p.out_chunk_rows;
	});
}

int gra_get_strip_plan_aa(gra_app *app, uint32_t *out12)
{
	return guarded(app, [&]() {
		if (!out12)
			throw std::logic_error("gra_get_strip_plan_aa: null output");
		auto &p = app->app->get_strip_plan();
		uint32_t *o = out12;
		for (const Granite::RowRange *r : {&p.taa, &p.smaa_edges, &p.smaa_weights, &p.aa_out})
		{
			*o++ = r->whole ? 1u : 0u;
			*o++ = r->first;
			*o++ = r->count;
		}
	});
}

int gra_get_strip_plan_taa_history(gra_app *app, uint32_t *out5)
{
	return guarded(app, [&]() {
		if (!out5)
			throw std::logic_error("gra_get_strip_plan_taa_history: null output");
		auto &p = app->app->get_strip_plan();
		out5[0] = p.aa.taa_history_reach;
		out5[1] = p.taa_exchange_rows;
		out5[2] = p.taa_history_held.whole ? 1u : 0u;
		out5[3] = p.taa_history_held.first;
		out5[4] = p.taa_history_held.count;
	});
}

int gra_get_host_stats(gra_app *app, double *out3)
{
	return guarded(app, [&]() {
		if (!out3)
			throw std::logic_error("gra_get_host_stats: null output");
		app->app->get_host_stats(out3);
	});
}

int gra_get_output_gather_stats(gra_app *app, uint64_t *out2)
{
	return guarded(app, [&]() {
		if (!out2)
			throw std::logic_error("gra_get_output_gather_stats: null output");
		app->app->get_output_gather_stats(out2);
	});
}

int gra_install_ssr_tables(const uint8_t *blue_noise_128x128_rg8, const uint16_t *brdf_lut_rg16f, uint32_t brdf_width, uint32_t brdf_height)
{
	try
	{
		Granite::ssr_install_tables(blue_noise_128x128_rg8, brdf_lut_rg16f, brdf_width, brdf_height);
		return 0;
	}
	catch (const std::exception &e)
	{
		fprintf(stderr, "gra_install_ssr_tables: %s\n", e.what());
		return -1;
	}
}

int gra_get_prefetched_refreshes(gra_app *app, uint64_t *out)
{
	return guarded(app, [&]() {
		if (!out)
			throw std::logic_error("gra_get_prefetched_refreshes: null output");
		*out = app->app->get_clusterer().get_prefetch_hits();
	});
}

int gra_get_launch_graph_replays(gra_app *app, uint64_t *out)
{
	return guarded(app, [&]() {
		if (!out)
			throw std::logic_error("gra_get_launch_graph_replays: null output");
		*out = app->app->get_device().get_launch_graph_replays();
	});
}

int gra_get_allocated_bytes(gra_app *app, uint64_t *out)
{
	return guarded(app, [&]() {
		if (!out)
			throw std::logic_error("gra_get_allocated_bytes: null output");
		*out = app->app->get_allocated_bytes();
	});
}

int gra_sync(gra_app *app)
{
	return guarded(app, [&]() {
		app->app->wait_idle();
		Granite::TimelineTrace::get().flush();
	});
}

static void fill_image_info(gra_resource_info *info, HIP::Image &img, int phys)
{
	info->device_ptr = img.get_device_pointer();
	info->width = img.get_width();
	info->height = img.get_height();
	info->format = img.get_format();
	info->size_bytes = img.get_size_bytes();
	info->physical_index = phys;
	info->levels = img.get_levels();
}

static void lookup_resource(gra_app *app, const char *name, gra_resource_info *info)
{
	auto &graph = app->app->get_graph();
	*info = {};
	// Buffers and textures share one name table; try texture first.
	try
	{
		auto &tex = graph.get_texture_resource(name);
		if (tex.get_physical_index() == RenderResource::Unused)
			throw std::logic_error(std::string("resource not part of the baked graph: ") + name);
		fill_image_info(info, graph.get_physical_texture_resource(tex), int(tex.get_physical_index()));
		return;
	}
	catch (const std::logic_error &)
	{
	}
	auto &buf = graph.get_buffer_resource(name);
	if (buf.get_physical_index() == RenderResource::Unused)
		throw std::logic_error(std::string("resource not part of the baked graph: ") + name);
	auto &phys = graph.get_physical_buffer_resource(buf);
	info->device_ptr = phys.get_device_pointer();
	info->size_bytes = phys.get_size();
	info->physical_index = int(buf.get_physical_index());
}

int gra_get_resource(gra_app *app, const char *name, gra_resource_info *info)
{
	return guarded(app, [&]() { lookup_resource(app, name, info); });
}

int gra_read_resource(gra_app *app, const char *name, void *dst_host, uint64_t size_bytes)
{
	return guarded(app, [&]() {
		gra_resource_info info;
		lookup_resource(app, name, &info);
		if (size_bytes > info.size_bytes)
			throw std::logic_error("read size exceeds resource size");
		app->app->wait_idle();
		auto *ctx = app->app->get_device().get_context();
		if (gr_download(ctx, nullptr, dst_host, info.device_ptr, size_bytes) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	});
}

int gra_write_resource(gra_app *app, const char *name, const void *src_host, uint64_t size_bytes)
{
	return guarded(app, [&]() {
		if (!src_host)
			throw std::logic_error("gra_write_resource: null source");
		app->app->prepare_resources_for_write();
		gra_resource_info info;
		lookup_resource(app, name, &info);
		if (size_bytes != info.size_bytes)
			throw std::logic_error("gra_write_resource: the size must be the resource's (" + std::to_string(info.size_bytes) + " bytes)");
		app->app->wait_idle();
		auto *ctx = app->app->get_device().get_context();
		if (gr_upload(ctx, nullptr, info.device_ptr, src_host, size_bytes) < 0 || gr_sync(ctx, nullptr) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	});
}

int gra_get_frame_state(gra_app *app, gra_frame_state *state)
{
	return guarded(app, [&]() {
		if (!state)
			throw std::logic_error("gra_get_frame_state: null argument");
		app->app->get_frame_state(*state);
	});
}

int gra_set_frame_state(gra_app *app, const gra_frame_state *state)
{
	return guarded(app, [&]() {
		if (!state)
			throw std::logic_error("gra_set_frame_state: null argument");
		app->app->set_frame_state(*state);
	});
}

int gra_save_resource_gtx(gra_app *app, const char *name, const char *path)
{
	return guarded(app, [&]() {
		if (!path)
			throw std::logic_error("gra_save_resource_gtx: null path");
		if (!name)
		{
			auto *bb = app->app->get_last_backbuffer();
			if (!bb)
				throw std::logic_error("no frame rendered yet");
			app->app->save_image_gtx(*bb, path);
			return;
		}
		auto &graph = app->app->get_graph();
		auto &tex = graph.get_texture_resource(name);
		app->app->save_image_gtx(graph.get_physical_texture_resource(tex), path);
	});
}

int gra_get_backbuffer(gra_app *app, gra_resource_info *info)
{
	return guarded(app, [&]() {
		auto *bb = app->app->get_last_backbuffer();
		if (!bb)
			throw std::logic_error("no frame rendered yet");
		fill_image_info(info, *bb, -1);
	});
}

int gra_read_backbuffer(gra_app *app, void *dst_host, uint64_t size_bytes)
{
	return guarded(app, [&]() {
		auto *bb = app->app->get_last_backbuffer();
		if (!bb)
			throw std::logic_error("no frame rendered yet");
		if (size_bytes > bb->get_size_bytes())
			throw std::logic_error("read size exceeds backbuffer size");
		app->app->wait_idle();
		auto *ctx = app->app->get_device().get_context();
		if (gr_download(ctx, nullptr, dst_host, bb->get_device_pointer(), size_bytes) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	});
}

int gra_get_cluster_state(gra_app *app, void *lights48, void *models48, uint32_t *type_mask128, void *params176, uint32_t *light_ranges)
{
	if (!app)
		return -1;
	try
	{
		auto &c = app->app->get_clusterer();
		auto &lights = c.get_packed_lights();
		if (lights48)
			memcpy(lights48, lights.data(), lights.size() * sizeof(lights[0]));
		if (models48)
			memcpy(models48, c.get_packed_models().data(), lights.size() * sizeof(mat_affine));
		if (type_mask128)
			memcpy(type_mask128, c.get_type_mask(), 128 * sizeof(uint32_t));
		if (params176)
			memcpy(params176, &c.get_cluster_parameters_bindless(), sizeof(ClustererParametersBindless));
		if (light_ranges)
			memcpy(light_ranges, c.get_volume_index_range().data(), c.get_volume_index_range().size() * sizeof(uvec2));
		return int(lights.size());
	}
	catch (const std::exception &e)
	{
		app->error = e.what();
		return -1;
	}
}

size_t gra_dump_graph(gra_app *app, char *buffer, size_t size)
{
	if (!app)
		return 0;
	std::string json;
	try
	{
		if (app->app->get_graph().get_baked_pass_order().empty())
			app->app->bake_only();
		json = app->app->get_graph().dump_json();
	}
	catch (const std::exception &e)
	{
		app->error = e.what();
		return 0;
	}
	if (buffer && size)
	{
		size_t n = std::min(size - 1, json.size());
		memcpy(buffer, json.data(), n);
		buffer[n] = '\0';
	}
	return json.size() + 1;
}

int gra_generate_mipmaps(gra_app *app, const void *level0_rgba16f, uint32_t width, uint32_t height, uint32_t levels,
                         uint32_t components, const float *filter_mods, void *chain_rgba16f)
{
	return guarded(app, [&]() {
		if (!level0_rgba16f || !chain_rgba16f || width == 0 || height == 0 || levels < 2 || levels > Granite::MaxSPDMips + 1)
			throw std::logic_error("gra_generate_mipmaps: bad argument");
		auto &device = app->app->get_device();
		device.wait_idle();
		auto image = device.create_image(width, height, VK_FORMAT_R16G16B16A16_SFLOAT, "mipmapped", levels);
		auto *ctx = device.get_context();
		auto stream = device.get_stream(HIP::CommandBuffer::Type::Generic);
		if (gr_upload(ctx, stream, image->get_device_pointer(), level0_rgba16f, size_t(width) * height * 8) < 0)
			throw std::runtime_error(gr_last_error(ctx));

		// The reference's use of the downsampler (renderer/ocean.cpp:579-601): level 0 is the source, levels 1.. the outputs.
		const gr_image source = image->get_level_view(0);
		std::vector<gr_image> views;
		std::vector<const gr_image *> mips;
		for (unsigned l = 1; l < levels; l++)
			views.push_back(image->get_level_view(l));
		for (auto &v : views)
			mips.push_back(&v);
		std::vector<Granite::vec4> mods;
		if (filter_mods)
			for (unsigned l = 0; l + 1 < levels; l++)
				mods.emplace_back(filter_mods[4 * l], filter_mods[4 * l + 1], filter_mods[4 * l + 2], filter_mods[4 * l + 3]);

		Granite::SPDInfo info = {};
		info.input = &source;
		info.output_mips = mips.data();
		info.num_mips = unsigned(mips.size());
		info.num_components = components;
		info.filter_mod = filter_mods ? mods.data() : nullptr;
		info.mode = Granite::ReductionMode::Color;
		HIP::CommandBuffer cmd{device, stream, HIP::CommandBuffer::Type::Generic};
		Granite::emit_single_pass_downsample(cmd, info);
		if (gr_download(ctx, stream, chain_rgba16f, image->get_device_pointer(), image->get_size_bytes()) < 0 || gr_sync(ctx, stream) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	});
}

int gra_reset_timestamps(gra_app *app)
{
	if (!app)
		return -1;
	try
	{
		app->app->get_graph().reset_timestamps();
		return 0;
	}
	catch (const std::exception &e)
	{
		app->error = e.what();
		return -1;
	}
}

int gra_set_directional_light(gra_app *app, const float direction[3], const float color[3])
{
	if (!app)
		return -1;
	if (!direction || !color)
	{
		app->error = "gra_set_directional_light: null argument";
		return -1;
	}
	app->app->set_directional_light(direction, color);
	return 0;
}

int gra_set_directional_shadows(gra_app *app, const gra_directional_shadows *desc)
{
	return guarded(app, [&]() { app->app->set_directional_shadows(desc); });
}

int gra_set_fog(gra_app *app, const float color[3], float falloff)
{
	if (!app)
		return -1;
	if (!color)
	{
		app->error = "gra_set_fog: null argument";
		return -1;
	}
	app->app->set_fog(color, falloff);
	return 0;
}

int gra_collect_timestamps(gra_app *app, gra_timestamp *entries, int max_entries)
{
	if (!app)
		return -1;
	try
	{
		auto reports = app->app->get_graph().collect_timestamps();
		int n = 0;
		for (auto &r : reports)
		{
			if (n >= max_entries)
				break;
			snprintf(entries[n].tag, sizeof(entries[n].tag), "%s", r.tag.c_str());
			entries[n].count = r.count;
			entries[n].total_ms = r.total_ms;
			n++;
		}
		return n;
	}
	catch (const std::exception &e)
	{
		app->error = e.what();
		return -1;
	}
}

int gra_get_taa_reprojection(gra_app *app, float *reproj16)
{
	return guarded(app, [&]() {
		mat4 m = app->app->get_taa_reprojection();
		memcpy(reproj16, m.data(), 16 * sizeof(float));
	});
}

int gra_set_smaa_luts(gra_app *app, const void *area_rg8, const void *search_r8)
{
	return guarded(app, [&]() {
		auto *ctx = app->app->get_device().get_context();
		if (gr_smaa_set_luts(ctx, area_rg8, search_r8) < 0)
			throw std::runtime_error(gr_last_error(ctx));
	});
}

void *gra_get_kernel_context(gra_app *app)
{
	return app ? app->app->get_device().get_context() : nullptr;
}

void *gra_get_stream(gra_app *app)
{
	return app ? app->app->get_device().get_stream(HIP::CommandBuffer::Type::Generic) : nullptr;
}
}

int gra_video_begin(gra_app *app, const gra_video_options *options)
{
	return guarded(app, [&]() {
		if (!options)
			throw std::logic_error("gra_video_begin: options are required");
		app->app->video_begin(*options);
	});
}

int gra_video_frame_layout(gra_app *app, gra_video_layout *layout)
{
	return guarded(app, [&]() {
		if (!layout)
			throw std::logic_error("gra_video_frame_layout: layout is required");
		*layout = app->app->video_layout();
	});
}

int gra_video_read_frame(gra_app *app, void *dst_host, uint64_t size_bytes, int64_t *frame_number)
{
	bool got = false;
	const int rc = guarded(app, [&]() {
		if (!dst_host)
			throw std::logic_error("gra_video_read_frame: destination is required");
		got = app->app->video_read(dst_host, size_bytes, frame_number);
	});
	return rc < 0 ? rc : (got ? 0 : 1);
}

int gra_video_end(gra_app *app)
{
	return guarded(app, [&]() { app->app->video_end(); });
}

int gra_video_play_begin(gra_app *app, const gra_video_play_options *options)
{
	return guarded(app, [&]() {
		if (!options)
			throw std::logic_error("gra_video_play_begin: options are required");
		app->app->video_play_begin(*options);
	});
}

int gra_video_play_layout(gra_app *app, gra_video_layout *layout)
{
	return guarded(app, [&]() {
		if (!layout)
			throw std::logic_error("gra_video_play_layout: layout is required");
		*layout = app->app->video_play_layout();
	});
}

int gra_video_play_frame(gra_app *app, const void *frame, uint64_t size_bytes)
{
	return guarded(app, [&]() {
		if (!frame)
			throw std::logic_error("gra_video_play_frame: frame is required");
		app->app->video_play_frame(frame, size_bytes);
	});
}

int gra_video_play_read_rgb(gra_app *app, void *dst_host, uint64_t size_bytes, int64_t *frame_number)
{
	bool got = false;
	const int rc = guarded(app, [&]() {
		if (!dst_host)
			throw std::logic_error("gra_video_play_read_rgb: destination is required");
		got = app->app->video_play_read(dst_host, size_bytes, frame_number);
	});
	return rc < 0 ? rc : (got ? 0 : 1);
}

int gra_video_play_end(gra_app *app)
{
	return guarded(app, [&]() { app->app->video_play_end(); });
}
