// Executor scheduling: see frame_schedule.hpp.
#include "frame_schedule.hpp"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

namespace Granite
{
const char *stream_name(StreamType stream)
{
	switch (stream)
	{
	case StreamType::Generic: return "generic";
	case StreamType::AsyncCompute: return "async";
	case StreamType::Front: return "front";
	case StreamType::Tail: return "tail";
	default: return "?";
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// Bake time: streams and hand-over rings
// ---------------------------------------------------------------------------------------------------------------------

// Frame pipelining (HIP executor policy, set_hoist_independent_compute): the "front" of a frame is every pass that
// does not depend, directly or through other passes, on anything carried over from the previous frame (history
// inputs, buffers that are read before they are written within the frame) -- cluster build, G-buffer, lighting.  The
// front runs on the second stream, so the front of frame N+1 executes while the back of frame N (bloom pyramid with
// its feedback, exposure, tonemap, AA) is still in flight on the first stream.
static std::vector<bool> find_front(const std::vector<StreamPlan::Pass> &passes, const std::vector<StreamPlan::Resource> &resources,
                                    const std::vector<StreamType> &pass_stream, unsigned swapchain)
{
	const size_t count = passes.size();
	std::vector<bool> front(count, false);
	std::vector<int> first_writer(resources.size(), -1), any_writer(resources.size(), 0);
	for (size_t i = 0; i < count; i++)
		for (unsigned w : passes[i].writes)
		{
			if (first_writer[w] < 0)
				first_writer[w] = int(i);
			any_writer[w]++;
		}
	std::vector<bool> written_by_back(resources.size(), false);
	bool any_back = false;
	for (size_t i = 0; i < count; i++)
	{
		auto &pass = passes[i];
		bool ok = pass_stream[i] == StreamType::Generic && !pass.has_history_inputs && !pass.writes.empty();
		for (unsigned w : pass.writes)
			ok = ok && w != swapchain && !resources[w].has_history;
		for (unsigned r : pass.reads)
		{
			// Every producer of what it reads must already have run in this frame, on the front.
			const bool produced_before = first_writer[r] >= 0 && first_writer[r] < int(i);
			const bool rmw_of_own_output = std::find(pass.writes.begin(), pass.writes.end(), r) != pass.writes.end();
			ok = ok && !written_by_back[r] && (produced_before || (any_writer[r] == 0)) && !(rmw_of_own_output && first_writer[r] == int(i));
		}
		front[i] = ok;
		if (!ok)
		{
			any_back = true;
			for (unsigned w : pass.writes)
				written_by_back[w] = true;
		}
	}
	if (!any_back) // nothing to overlap with: keep the whole frame on one stream
		front.assign(count, false);
	return front;
}

// The tail: the longest run of passes at the end of the baked order that (a) stand on the generic stream, (b) write nothing the next
// frame reads (no image with history, nothing read before it is written within the frame: bloom's feedback, exposure) and (c) whose
// first pass -- and with it the whole run -- takes exactly ONE physical resource from the passes in front of it.  For the application's
// graphs that is post-tonemap anti-aliasing reading `tonemapped`; a frame that ends with the tonemap has no tail.  Frame N's tail then
// runs beside frame N + 1's back instead of in front of it (the passes of the tail depend on nothing frame N + 1 produces and
// produce nothing it consumes): TAA resolve N + 1 no longer queues behind SMAA N.  Returns where the run begins: the number of passes where there is none.
static size_t find_tail(const std::vector<StreamPlan::Pass> &passes, const std::vector<StreamPlan::Resource> &resources,
                        const std::vector<StreamType> &pass_stream, unsigned swapchain)
{
	const size_t count = passes.size();
	std::vector<bool> carried(resources.size(), false); // read by some pass before any pass of the frame has written it
	{
		std::vector<bool> written(resources.size(), false);
		for (auto &pass : passes)
		{
			for (unsigned r : pass.reads)
				if (!written[r])
					carried[r] = true;
			for (unsigned w : pass.writes)
				written[w] = true;
		}
	}
	// the longest suffix satisfying (a) and (b)
	size_t begin = count;
	while (begin > 0)
	{
		auto &pass = passes[begin - 1];
		bool ok = pass_stream[begin - 1] == StreamType::Generic && !pass.has_history_inputs && !pass.conditional;
		for (unsigned w : pass.writes)
			ok = ok && !resources[w].has_history && !carried[w] && !resources[w].is_buffer;
		if (!ok)
			break;
		begin--;
	}
	// (c): shrink from the front until what crosses into the run is one image, written once, by a back pass
	for (; begin < count; begin++)
	{
		std::vector<bool> inside(resources.size(), false);
		for (size_t i = begin; i < count; i++)
			for (unsigned w : passes[i].writes)
				inside[w] = true;
		std::vector<unsigned> crossing;
		for (size_t i = begin; i < count; i++)
			for (unsigned r : passes[i].reads)
				if (!inside[r] && std::find(crossing.begin(), crossing.end(), r) == crossing.end())
					crossing.push_back(r);
		if (crossing.size() != 1)
			continue;
		unsigned writers = 0;
		bool back_writer = true;
		for (size_t i = 0; i < begin; i++)
			for (unsigned w : passes[i].writes)
				if (w == crossing[0])
				{
					writers++;
					back_writer = back_writer && pass_stream[i] == StreamType::Generic;
				}
		if (writers == 1 && back_writer && !resources[crossing[0]].is_buffer && !resources[crossing[0]].has_history && !carried[crossing[0]] &&
		    crossing[0] != swapchain)
			break;
	}
	// ... and something must be left in front of it on the generic stream for the run to overlap with
	bool back_in_front = false;
	for (size_t i = 0; i < begin && i < count; i++)
		back_in_front = back_in_front || pass_stream[i] == StreamType::Generic;
	return back_in_front ? begin : count;
}

void StreamPlan::build(std::vector<Pass> baked_passes, const std::vector<Resource> &resources, unsigned swapchain, unsigned blit_source,
                       const Options &options)
{
	passes = std::move(baked_passes);
	const size_t count = passes.size();
	pass_stream.assign(count, StreamType::Generic);
	for (size_t i = 0; i < count; i++)
		if (passes[i].async_compute_queue)
			pass_stream[i] = StreamType::AsyncCompute;
	uses_async_stream = false;

	std::vector<bool> front(count, false);
	if (options.hoist_independent_compute)
		front = find_front(passes, resources, pass_stream, swapchain);
	for (size_t i = 0; i < count; i++)
	{
		if (front[i])
			pass_stream[i] = passes[i].reads.empty() ? StreamType::AsyncCompute : StreamType::Front;
		uses_async_stream = uses_async_stream || pass_stream[i] != StreamType::Generic;
	}

	// (a frame that ends in a blit to the swapchain keeps its end on the generic stream, where the blit is)
	if (options.hoist_independent_compute && options.split_tail && uses_async_stream && swapchain != Unused)
		for (size_t i = find_tail(passes, resources, pass_stream, swapchain); i < count; i++)
			pass_stream[i] = StreamType::Tail;

	// Which streams read and write each resource, and how many passes write it.
	std::vector<unsigned> writers(resources.size(), 0);
	std::vector<uint8_t> reader_streams(resources.size(), 0), writer_streams(resources.size(), 0);
	for (size_t i = 0; i < count; i++)
	{
		for (unsigned w : passes[i].writes)
		{
			writers[w]++;
			writer_streams[w] |= stream_bit(pass_stream[i]);
		}
		for (unsigned r : passes[i].reads)
			reader_streams[r] |= stream_bit(pass_stream[i]);
	}
	if (blit_source != Unused)
		reader_streams[blit_source] |= stream_bit(StreamType::Generic); // final blit runs on the generic stream

	// Only passes that touch a resource which is also touched from the other stream take part in event ordering; every
	// other pass is ordered by its in-order stream alone and records nothing (event / barrier packets are not free:
	// each one is a command-processor round trip between two kernels).
	pass_needs_sync.assign(count, false);
	blit_needs_sync = false;
	if (uses_async_stream)
	{
		auto several_streams_touch = [&](unsigned resource) {
			const uint8_t bits = reader_streams[resource] | writer_streams[resource];
			return (bits & (bits - 1)) != 0;
		};
		blit_needs_sync = blit_source != Unused && several_streams_touch(blit_source);
		for (size_t i = 0; i < count; i++)
		{
			bool shared = false;
			for (unsigned r : passes[i].reads)
				shared = shared || several_streams_touch(r);
			for (unsigned w : passes[i].writes)
				shared = shared || several_streams_touch(w);
			// The front's stream alternates with the frame's parity (HIP::Device): what two front passes of different frames share (the
			// G-buffer targets a producer pass rewrites three frames after the lighting pass read them) is ordered by events too.
			pass_needs_sync[i] = shared || (pass_stream[i] == StreamType::Front && options.front_alternates);
		}
	}

	// What the front writes and the back reads exists twice and alternates per frame (like an image with history), so the
	// front of frame N+1 never waits for the back of frame N to finish reading: write-after-read across frames disappears.
	// Only resources with a single writer qualify (every byte the back reads is rewritten by the front each frame).
	physical_buffer_double.assign(resources.size(), false);
	const bool has_tail = std::find(pass_stream.begin(), pass_stream.end(), StreamType::Tail) != pass_stream.end();
	for (size_t i = 0; i < count; i++)
	{
		// ... and what the back hands to the tail (`tonemapped`), for the same reason one stage further down the frame
		const bool hands_to_tail = has_tail && pass_stream[i] == StreamType::Generic;
		if (front[i] || hands_to_tail)
			for (unsigned w : passes[i].writes)
			{
				const uint8_t others = reader_streams[w] & ~stream_bit(pass_stream[i]);
				if (writers[w] == 1 && (front[i] ? others != 0 : (others & stream_bit(StreamType::Tail)) != 0))
					physical_buffer_double[w] = true;
			}
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// Per frame: cross-stream hazards
// ---------------------------------------------------------------------------------------------------------------------
static const bool sync_debug = getenv("GRANITE_SYNC_DEBUG") != nullptr;

HazardTracker::~HazardTracker()
{
	for (void *e : pass_done_event)
		if (e)
			(void)hipEventDestroy(static_cast<hipEvent_t>(e));
}

void HazardTracker::reset(std::vector<std::string> resource_names_, std::vector<std::string> pass_names_)
{
	resource_names = std::move(resource_names_);
	pass_names = std::move(pass_names_);
	sync.assign(resource_names.size(), {});
	for (auto &v : sync_alternate)
		v.assign(resource_names.size(), {});
}

void HazardTracker::begin_frame(HIP::Device &device_, size_t pass_count, bool blit_follows_)
{
	device = &device_;
	ring_slot = size_t(frame_counter++ % EventRing);
	// rows 1 .. (number of runs <= number of passes); row 0 belongs to the final blit
	if (pass_done_event.size() < (pass_count + 1) * EventRing)
		pass_done_event.resize((pass_count + 1) * EventRing, nullptr);
	this_frame = frame_counter - 1;
	// The runs published under the device's frame fences stay named for EventRing frames on the assumption that the device's ring and this
	// one advance together: one next_frame_context() per enqueued frame.  A caller that rotates the device faster only makes waits
	// stricter (a fence re-recorded early is a later point of its stream), i.e. costs barrier packets, never correctness: say so once.
	if (sync_debug && last_device_frame != 0 && device_.get_frame_number() != last_device_frame + 1)
	{
		static bool told = false;
		if (!told)
			fprintf(stderr, "[sync] the device advanced %llu frame contexts between two enqueued frames: published fences are re-recorded early (stricter waits)\n",
			        (unsigned long long)(device_.get_frame_number() - last_device_frame));
		told = true;
	}
	last_device_frame = device_frame = device_.get_frame_number();
	device_completed = device_.get_completed_frame();
	blit_follows = blit_follows_;
	expected_runs = 0;
	expected_stream = run_stream = StreamType::Count;
	std::fill(std::begin(last_run_of_stream), std::end(last_run_of_stream), -1);
	run_slot = 0;
	run_published = false;
	current_pass = -1;
	waited.clear();
}

// The last run a frame puts on a stream publishes under the DEVICE's fence of that stream and frame (the staging ring's, same depth as
// EventRing) and records it here: the fence next_frame_context() would otherwise record right behind the run's own event.
// Which run that is: a dry pass over the frame's passes (need_render_pass is asked once per pass and frame).
void HazardTracker::expect_pass(StreamType stream)
{
	if (stream != expected_stream)
	{
		expected_stream = stream;
		expected_runs++;
	}
	last_run_of_stream[int(stream)] = expected_runs;
}

void HazardTracker::enter_pass(StreamType stream, int pass)
{
	if (stream != run_stream)
		open_run(stream, run_slot + 1);
	current_pass = pass;
}

void HazardTracker::enter_blit()
{
	open_run(StreamType::Generic, 0);
	current_pass = -1;
}

void HazardTracker::open_run(StreamType stream, unsigned slot)
{
	close_run();
	run_stream = stream;
	run_slot = slot;
	waited.clear();
}

void *HazardTracker::run_event()
{
	// (the final blit goes behind the generic stream's last run: that run keeps its own event, the fence is recorded behind the blit)
	if (int(run_slot) == last_run_of_stream[int(run_stream)] && !(blit_follows && run_stream == StreamType::Generic))
		return device->frame_fence(run_stream);
	void *&event = pass_done_event[run_slot * EventRing + ring_slot];
	if (!event)
	{
		hipEvent_t e;
		// ordering between streams of this device only: no system-scope fence (GRANITE_SYNC_EVENT_SYSTEM_FENCE=1 restores it)
		static const unsigned flags = hipEventDisableTiming | (getenv("GRANITE_SYNC_EVENT_SYSTEM_FENCE") ? 0u : unsigned(hipEventDisableSystemFence));
		if (hipEventCreateWithFlags(&e, flags) != hipSuccess)
			throw std::runtime_error("hipEventCreate failed");
		event = e;
	}
	return event;
}

void HazardTracker::close_run()
{
	if (run_stream != StreamType::Count && run_published)
	{
		void *event = run_event();
		if (event == device->frame_fence(run_stream))
			device->record_frame_fence(run_stream);
		else if (hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(device->get_stream(run_stream))) != hipSuccess)
			throw std::runtime_error("hipEventRecord failed");
	}
	run_published = false;
}

void HazardTracker::wait_for(const Access &access, const char *kind, unsigned resource)
{
	if (!access.event || std::find(waited.begin(), waited.end(), access.event) != waited.end())
		return;
	// recorded in a frame the host has already waited for (frame pacing: three frames back with the default lead): complete, no call at all
	// -- the write-after-read dependencies on the rotating copies' previous users are all of this kind
	if (access.device_frame != 0 && access.device_frame <= device_completed)
		return;
	waited.push_back(access.event);
	// The host runs one to two frames ahead of the GPU (Device::next_frame_context), so most cross-stream dependencies (anything on work of two
	// frames ago, usually the cluster build as well) are already complete when they are looked at: no barrier packet
	// is needed then, and each one costs the command processor several microseconds between two kernels.
	if (hipEventQuery(static_cast<hipEvent_t>(access.event)) == hipSuccess)
		return;
	if (sync_debug)
		fprintf(stderr, "[sync] frame %llu pass %s waits %s on %s: pass %s of frame %llu\n", (unsigned long long)this_frame,
		        current_pass >= 0 ? pass_names[current_pass].c_str() : "blit", kind, resource_names[resource].c_str(),
		        access.pass >= 0 && access.pass < int(pass_names.size()) ? pass_names[access.pass].c_str() : "?", (unsigned long long)access.frame);
	if (hipStreamWaitEvent(static_cast<hipStream_t>(device->get_stream(run_stream)), static_cast<hipEvent_t>(access.event), 0) != hipSuccess)
		throw std::runtime_error("cross-queue dependency failed");
}

// RAW / WAW / WAR against accesses recorded on the other stream.
// (An access of the same stream type is ordered by the stream itself -- unless the type's stream alternates with the frame's parity, the
// front's, and the access was recorded in a frame of the other parity: the device says, frame numbers being the device's.)
void HazardTracker::acquire(const std::vector<unsigned> &reads, const std::vector<unsigned> &writes)
{
	auto in_order_with = [&](const Access &access) {
		return access.stream == run_stream && device->same_stream(run_stream, device_frame, access.device_frame);
	};
	for (unsigned r : reads)
		if (!in_order_with(sync[r].write))
			wait_for(sync[r].write, "RAW", r);
	for (unsigned w : writes)
	{
		if (!in_order_with(sync[w].write))
			wait_for(sync[w].write, "WAW", w);
		for (auto &read : sync[w].read)
			if (!in_order_with(read))
				wait_for(read, "WAR", w);
	}
}

void HazardTracker::release(const std::vector<unsigned> &reads, const std::vector<unsigned> &writes)
{
	const Access access = {run_event(), current_pass, this_frame, device_frame, run_stream};
	for (unsigned r : reads)
		sync[r].read[int(run_stream)] = access;
	for (unsigned w : writes)
	{
		sync[w].write = access;
		for (auto &read : sync[w].read)
			read = {};
	}
	run_published = true;
}
} // namespace Granite
