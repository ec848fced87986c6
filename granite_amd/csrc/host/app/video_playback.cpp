// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Frame playback of ImageSpaceApplication: what VideoDecoder does with a decoded frame (ffmpeg_decode.cpp: upload of the planes,
// dispatch_conversion), minus demuxer and decoder.  The caller hands over packed frames in the layout recording produces; each one is
// copied into a pinned ring slot, uploaded and converted on the player's own stream, and its RGB image copied back into the slot.
//
// Ordering, without a device sync:
//   * upload N, conversion N and read-back N are in order on the player's stream, and so are frames N and N + 1: one device copy of
//     the planes and one of the RGB image suffice;
//   * a ring slot's pinned buffers are reused only after gra_video_play_read_rgb handed the frame back, which waited for that
//     frame's event (a full ring fails the next gra_video_play_frame instead): the host never writes a buffer a copy still reads.
#include "image_space_app.hpp"
#include <hip/hip_runtime_api.h>
#include <cstring>
#include <stdexcept>

namespace Granite
{
namespace
{
uint32_t rgb_texel_bytes(uint32_t format)
{
	switch (format)
	{
	case GR_FORMAT_R8G8B8A8_UNORM:
	case GR_FORMAT_R8G8B8A8_SRGB:
	case GR_FORMAT_A2B10G10R10_UNORM_PACK32: return 4;
	case GR_FORMAT_R16G16B16A16_SFLOAT: return 8;
	default: return 0;
	}
}
} // namespace

void ImageSpaceApplication::video_play_begin(const gra_video_play_options &options)
{
	if (playback)
		throw std::logic_error("gra_video_play_begin: already playing");
	if (config.strip_count > 1)
		throw std::logic_error("gra_video_play_begin: playback with row bands (strip_count > 1) is not supported");
	if (!options.width || !options.height)
		throw std::logic_error("gra_video_play_begin: width and height are required");
	auto play = std::make_unique<VideoPlayback>();
	play->options = options;
	if (!video_format_layout(options.format, options.width, options.height, play->layout, play->plane_format))
		throw std::logic_error("gra_video_play_begin: unknown format");
	const uint32_t texel = rgb_texel_bytes(options.output_format);
	if (!texel)
		throw std::logic_error("gra_video_play_begin: output format must be R8G8B8A8_{UNORM,SRGB}, A2B10G10R10_UNORM_PACK32 or R16G16B16A16_SFLOAT");
	const gra_video_layout &l = play->layout;
	play->rgb_pitch = options.width * texel;
	play->rgb_bytes = uint64_t(play->rgb_pitch) * options.height;

	// The conversion's arguments are checked now, not at the first frame (gr_video_yuv_plan needs no device).
	gr_image planes[3] = {};
	for (uint32_t i = 0; i < l.num_planes; i++)
		planes[i] = {nullptr, l.width[i], l.height[i], l.pitch[i], play->plane_format[i]};
	const gr_image out = {nullptr, options.width, options.height, play->rgb_pitch, options.output_format};
	play->converter.init(planes, l.num_planes, out, options.info);

	auto &device = get_device();
	device.make_current();
	playback = std::move(play); // from here on video_play_release() undoes what follows
	try
	{
		VideoRing &ring = playback->ring;
		ring.create("video playback", options.ring_frames ? options.ring_frames : 8u, l.frame_bytes, playback->rgb_bytes);
		ring.check(hipMalloc(&playback->planes, l.frame_bytes), "hipMalloc");
		ring.check(hipMalloc(&playback->rgb, playback->rgb_bytes), "hipMalloc");
	}
	catch (...)
	{
		video_play_release();
		throw;
	}
}

void ImageSpaceApplication::video_play_release()
{
	if (!playback)
		return;
	playback->ring.release();
	if (playback->planes)
		(void)hipFree(playback->planes);
	if (playback->rgb)
		(void)hipFree(playback->rgb);
	playback.reset();
}

void ImageSpaceApplication::video_play_end()
{
	if (!playback)
		throw std::logic_error("gra_video_play_end: not playing");
	video_play_release();
}

const gra_video_layout &ImageSpaceApplication::video_play_layout() const
{
	if (!playback)
		throw std::logic_error("gra_video_play_layout: not playing");
	return playback->layout;
}

void ImageSpaceApplication::video_play_frame(const void *frame, uint64_t size)
{
	if (!playback)
		throw std::logic_error("gra_video_play_frame: not playing");
	const gra_video_layout &l = playback->layout;
	if (size != l.frame_bytes)
		throw std::logic_error("gra_video_play_frame: size is not one frame's (gra_video_play_layout)");
	VideoRing &ring = playback->ring;
	if (ring.full())
		throw std::runtime_error("video playback: " + std::to_string(ring.slots.size()) +
		                         " converted frames are unread; read them with gra_video_play_read_rgb before playing more");
	auto &device = get_device();
	device.make_current();
	hipStream_t stream = ring.stream;
	VideoRing::Slot &slot = ring.next_slot();
	memcpy(slot.host[0], frame, l.frame_bytes);
	ring.check(hipMemcpyAsync(playback->planes, slot.host[0], l.frame_bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");

	gr_image planes[3] = {};
	for (uint32_t i = 0; i < l.num_planes; i++)
		planes[i] = {static_cast<uint8_t *>(playback->planes) + l.offset[i], l.width[i], l.height[i], l.pitch[i], playback->plane_format[i]};
	const gr_image out = {playback->rgb, playback->options.width, playback->options.height, playback->rgb_pitch, playback->options.output_format};
	playback->converter.convert(device.get_context(), stream, planes, out);

	ring.check(hipMemcpyAsync(slot.host[1], playback->rgb, playback->rgb_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
	ring.commit_slot();
}

bool ImageSpaceApplication::video_play_read(void *dst, uint64_t size, int64_t *frame_number)
{
	if (!playback)
		throw std::logic_error("gra_video_play_read_rgb: not playing");
	if (playback->ring.read == playback->ring.written)
		return false;
	if (size < playback->rgb_bytes)
		throw std::logic_error("gra_video_play_read_rgb: destination smaller than one image (width x height texels, tightly packed)");
	playback->ring.read_into(dst, 1, frame_number);
	return true;
}
} // namespace Granite
