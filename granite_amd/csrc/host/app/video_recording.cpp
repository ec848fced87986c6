// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen): see THIRD_PARTY_NOTICES.md at the repository root.
// Frame recording of ImageSpaceApplication: the headless runner's --video-encode-path (application_headless.cpp:225-275, 348-372)
// with VideoEncoder::create_ycbcr_pipeline + process_rgb (ffmpeg_encode.cpp), minus the encoder.  Every frame's swapchain image goes
// through VideoScaler::rescale on the recorder's stream and is copied into a ring of pinned host frames.
//
// Ordering, without a device sync:
//   * the conversion of frame N waits for the frame fences of every executor stream frame N was given work on (Device::
//     for_each_fence_of): whichever stream wrote the swapchain image last -- the generic stream's blit or tonemap, or the tail
//     stream's SMAA / FXAA when split_tail is on -- is among them;
//   * the swapchain image comes round again four frames later: before that frame enqueues anything, every executor stream waits for
//     the event recorded behind the conversion that read the image (queried first: normally long complete, then no wait is queued);
//   * conversion N + 1 and copy N share the in-order recorder stream, so one device copy of the planes suffices; the host copy of a
//     ring slot is reused only after gra_video_read_frame handed it back (a full ring fails the next frame instead).
#include "image_space_app.hpp"
#include <hip/hip_runtime_api.h>
#include <cstring>
#include <stdexcept>

namespace Granite
{
bool ImageSpaceApplication::video_format_layout(uint32_t f, uint32_t w, uint32_t h, gra_video_layout &l, uint32_t (&plane_format)[3])
{
	if (f > GRA_VIDEO_P016)
		return false;
	const bool wide = f == GRA_VIDEO_YUV420P16 || f == GRA_VIDEO_YUV444P16 || f == GRA_VIDEO_P010 || f == GRA_VIDEO_P016;
	const bool sub = f != GRA_VIDEO_YUV444P && f != GRA_VIDEO_YUV444P16;
	const bool two = f == GRA_VIDEO_NV12 || f == GRA_VIDEO_P010 || f == GRA_VIDEO_P016;
	const uint32_t cw = sub ? (w + 1) / 2 : w, ch = sub ? (h + 1) / 2 : h;
	const uint32_t bps = wide ? 2u : 1u;
	l = {};
	l.num_planes = two ? 2u : 3u;
	l.bytes_per_sample = bps;
	l.width[0] = w;
	l.height[0] = h;
	l.pitch[0] = w * bps;
	plane_format[0] = wide ? GR_FORMAT_R16_UNORM : GR_FORMAT_R8_UNORM;
	for (uint32_t i = 1; i < l.num_planes; i++)
	{
		l.width[i] = cw;
		l.height[i] = ch;
		l.pitch[i] = cw * bps * (two ? 2u : 1u);
		plane_format[i] = two ? (wide ? GR_FORMAT_R16G16_UNORM : GR_FORMAT_R8G8_UNORM) : plane_format[0];
	}
	uint64_t offset = 0;
	for (uint32_t i = 0; i < l.num_planes; i++)
	{
		l.offset[i] = offset;
		offset += uint64_t(l.pitch[i]) * l.height[i];
	}
	l.frame_bytes = offset;
	return true;
}

void ImageSpaceApplication::video_begin(const gra_video_options &options)
{
	if (video)
		throw std::logic_error("gra_video_begin: already recording");
	if (config.strip_count > 1)
		throw std::logic_error("gra_video_begin: recording with row bands (strip_count > 1) is not supported");
	if (options.format > GRA_VIDEO_P016)
		throw std::logic_error("gra_video_begin: unknown format");
	auto &device = get_device();
	device.make_current();

	auto rec = std::make_unique<VideoRecording>();
	rec->options = options;
	const uint32_t w = options.width ? options.width : config.width;
	const uint32_t h = options.height ? options.height : config.height;
	video_format_layout(options.format, w, h, rec->layout, rec->plane_format);
	gra_video_layout &l = rec->layout;

	// The conversion's arguments are checked now, not at the first frame (gr_video_scale_plan needs no device).
	gr_image input = {nullptr, config.width, config.height, config.width * 4u, uint32_t(backbuffer_format())};
	gr_image planes[3] = {};
	for (uint32_t i = 0; i < l.num_planes; i++)
		planes[i] = {nullptr, l.width[i], l.height[i], l.pitch[i], rec->plane_format[i]};
	gr_video_plan plan;
	const uint32_t in_space = config.hdr10 ? GR_COLOR_SPACE_HDR10_ST2084 : GR_COLOR_SPACE_SRGB_NONLINEAR;
	const uint32_t out_space = options.hdr10 ? GR_COLOR_SPACE_HDR10_ST2084 : GR_COLOR_SPACE_SRGB_NONLINEAR;
	if (gr_video_scale_plan(&input, planes, l.num_planes, in_space, out_space, &plan) < 0)
		throw std::logic_error("gra_video_begin: the conversion is not supported for these sizes / formats");

	video = std::move(rec); // from here on video_release() undoes what follows
	try
	{
		video->ring.create("video recording", options.ring_frames ? options.ring_frames : 8u, l.frame_bytes);
		video->ring.check(hipMalloc(&video->planes, l.frame_bytes), "hipMalloc");
	}
	catch (...)
	{
		video_release();
		throw;
	}
}

void ImageSpaceApplication::video_release()
{
	if (!video)
		return;
	video->ring.release();
	for (auto &e : video->read_done)
		(void)hipEventDestroy(static_cast<hipEvent_t>(e.second));
	if (video->planes)
		(void)hipFree(video->planes);
	video.reset();
}

void ImageSpaceApplication::video_end()
{
	if (!video)
		throw std::logic_error("gra_video_end: not recording");
	// the executor's streams may still wait for read_done events recorded on the recorder's stream: drain both before destroying them
	get_device().wait_idle();
	video_release();
}

const gra_video_layout &ImageSpaceApplication::video_layout() const
{
	if (!video)
		throw std::logic_error("gra_video_frame_layout: not recording");
	return video->layout;
}

void ImageSpaceApplication::video_check_ring() const
{
	if (video->ring.full())
		throw std::runtime_error("video recording: " + std::to_string(video->ring.slots.size()) +
		                         " recorded frames are unread; read them with gra_video_read_frame before rendering more");
}

void ImageSpaceApplication::video_before_frame(HIP::Image &backbuffer)
{
	auto itr = video->read_done.find(backbuffer.get_device_pointer());
	if (itr == video->read_done.end())
		return;
	auto done = static_cast<hipEvent_t>(itr->second);
	if (hipEventQuery(done) == hipSuccess)
		return;
	// the conversion that read this swapchain image four frames ago is still running: no stream of this frame may write it before
	auto &device = get_device();
	for (int i = 0; i < int(HIP::CommandBuffer::Type::Count); i++)
		video->ring.check(hipStreamWaitEvent(static_cast<hipStream_t>(device.get_stream(HIP::CommandBuffer::Type(i))), done, 0), "hipStreamWaitEvent");
}

void ImageSpaceApplication::video_after_frame(HIP::Image &backbuffer, uint64_t device_frame)
{
	auto &device = get_device();
	VideoRing &ring = video->ring;
	hipStream_t stream = ring.stream;
	device.for_each_fence_of(device_frame, [&](void *fence) {
		ring.check(hipStreamWaitEvent(stream, static_cast<hipEvent_t>(fence), 0), "hipStreamWaitEvent");
	});

	const gra_video_layout &l = video->layout;
	gr_image planes[3] = {};
	VideoScaler::RescaleInfo info = {};
	for (uint32_t i = 0; i < l.num_planes; i++)
	{
		planes[i] = {static_cast<uint8_t *>(video->planes) + l.offset[i], l.width[i], l.height[i], l.pitch[i], video->plane_format[i]};
		info.output_planes[i] = &planes[i];
	}
	const gr_image input = backbuffer.get_view();
	info.num_output_planes = l.num_planes;
	info.input = &input;
	info.input_color_space = config.hdr10 ? GR_COLOR_SPACE_HDR10_ST2084 : GR_COLOR_SPACE_SRGB_NONLINEAR;
	info.output_color_space = video->options.hdr10 ? GR_COLOR_SPACE_HDR10_ST2084 : GR_COLOR_SPACE_SRGB_NONLINEAR;
	video->scaler.rescale(device.get_context(), stream, info);

	void *&done = video->read_done[backbuffer.get_device_pointer()];
	if (!done)
	{
		hipEvent_t e;
		ring.check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreateWithFlags");
		done = e;
	}
	ring.check(hipEventRecord(static_cast<hipEvent_t>(done), stream), "hipEventRecord");

	ring.check(hipMemcpyAsync(ring.next_slot().host[0], video->planes, l.frame_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
	ring.commit_slot();
}

bool ImageSpaceApplication::video_read(void *dst, uint64_t size, int64_t *frame_number)
{
	if (!video)
		throw std::logic_error("gra_video_read_frame: not recording");
	if (video->ring.read == video->ring.written)
		return false;
	if (size < video->layout.frame_bytes)
		throw std::logic_error("gra_video_read_frame: destination smaller than one frame (gra_video_frame_layout)");
	video->ring.read_into(dst, 0, frame_number);
	return true;
}
} // namespace Granite
