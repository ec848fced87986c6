// The HIP executor's own scheduling policy (no counterpart in the reference, which decides queues at declaration time and orders them
// with barriers and semaphores): which of the four in-order streams a baked pass goes to and which resources become hand-over rings
// (StreamPlan, bake time, no HIP call), and the event waits that order the streams against each other while a frame is enqueued
// (HazardTracker).  Granite::RenderGraph (render_graph.hpp) feeds both; neither knows it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "hip_device.hpp"

namespace Granite
{
// A stream is named by the type of the command buffers recorded on it: generic (the back of the frame), async compute (passes the front
// does not wait for within a frame: explicit ASYNC_COMPUTE passes and input-free front passes such as the cluster build), front (the rest
// of the front), tail (what follows the frame's last pass with a tie to the next frame and reads one image of it).
using StreamType = HIP::CommandBuffer::Type;
enum { StreamCount = int(StreamType::Count) };
const char *stream_name(StreamType stream); // "generic", "async", "front", "tail": what graph dumps print
inline uint8_t stream_bit(StreamType stream) { return uint8_t(1u << int(stream)); } // for sets of streams

// HandOverCopies - 1 spare copies per resource; every frame the current copy goes to the back of the ring and the oldest
// spare becomes current.  Three copies: the producer of frame N+1 writes what the consumers of frame N-2 read last, so
// a back-of-frame that runs late (it shares the chip with the next frame's lighting) never stalls the front.
enum { HandOverCopies = 3 };
// rotate: current -> newest spare, oldest spare -> current
template <typename T>
void rotate_hand_over(std::vector<T> &current, std::vector<T> (&spares)[HandOverCopies - 1], size_t index)
{
	constexpr int count = HandOverCopies - 1;
	T previous = current[index];
	current[index] = spares[0][index];
	for (int k = 0; k + 1 < count; k++)
		spares[k][index] = spares[k + 1][index];
	spares[count - 1][index] = previous;
}

struct StreamPlan
{
	enum { Unused = ~0u };
	struct Pass // in baked order
	{
		std::vector<unsigned> reads, writes; // physical resources
		bool async_compute_queue = false;
		bool has_history_inputs = false;
		bool conditional = false; // may be skipped in a frame
	};
	struct Resource
	{
		bool is_buffer = false;
		bool has_history = false;
	};
	struct Options
	{
		bool hoist_independent_compute = true;
		bool split_tail = true;
		bool front_alternates = false; // HIP::Device::front_alternates()
	};
	// swapchain: the physical resource that is the swapchain image; blit_source: the one the final blit copies from; either is Unused
	void build(std::vector<Pass> baked_passes, const std::vector<Resource> &resources, unsigned swapchain, unsigned blit_source, const Options &options);

	std::vector<Pass> passes;
	std::vector<StreamType> pass_stream;
	std::vector<bool> pass_needs_sync; // touches a physical resource that another stream also touches
	bool blit_needs_sync = false;
	bool uses_async_stream = false; // some pass left the generic stream: with a single stream in use nothing is recorded
	// Resources written on one stream and read on another exist HandOverCopies times and rotate per frame (like an image with history), so
	// the hoisted pass of frame N+1 never waits for frame N's consumers: write-after-read across frames disappears.
	std::vector<bool> physical_buffer_double;
};

// Cross-stream ordering while a frame is enqueued.  Every pass that shares a resource with a pass on ANOTHER stream waits on that
// pass's "done" event (RAW, WAW and WAR); the state survives across frames, which is what lets frame N+1's hoisted passes start
// as soon as frame N's readers of their outputs have finished.
class HazardTracker
{
public:
	HazardTracker() = default;
	~HazardTracker(); // destroys the events it created
	HazardTracker(const HazardTracker &) = delete;
	void operator=(const HazardTracker &) = delete;

	// At bake: forget every access.  The names (resources by physical index, passes in baked order) are for GRANITE_SYNC_DEBUG=1.
	void reset(std::vector<std::string> resource_names, std::vector<std::string> pass_names);
	// A hand-over ring's resource moves on to its next copy: so does what is known about its accesses.
	void rotate(size_t resource) { rotate_hand_over(sync, sync_alternate, resource); }

	void begin_frame(HIP::Device &device, size_t pass_count, bool blit_follows);
	// Before the first enter_pass(): every pass this frame will run, in order (which run is the last a stream sees this frame).
	void expect_pass(StreamType stream);
	// The pass about to be enqueued: closes the run of passes in front of it if that stood on another stream.
	void enter_pass(StreamType stream, int pass);
	// The final blit, on the generic stream, a run of its own behind every pass (ring row 0).
	void enter_blit();
	// RAW / WAW / WAR: makes the current run's stream wait for accesses recorded on other streams.
	void acquire(const std::vector<unsigned> &reads, const std::vector<unsigned> &writes);
	// Publishes the current pass's accesses under the run's event.
	void release(const std::vector<unsigned> &reads, const std::vector<unsigned> &writes);
	void end_frame() { close_run(); }

private:
	struct Access
	{
		void *event = nullptr; // hipEvent_t
		// who recorded it (pass in baked order or -1 for the blit, frame), for GRANITE_SYNC_DEBUG=1 traces
		int pass = -1;
		uint64_t frame = 0;
		// the device's frame number at the record: which of a type's alternating streams it went to (HIP::Device::same_stream)
		uint64_t device_frame = 0;
		StreamType stream = StreamType::Count;
	};
	struct PhysicalSync
	{
		Access write, read[StreamCount];
	};
	std::vector<PhysicalSync> sync, sync_alternate[HandOverCopies - 1];
	std::vector<std::string> resource_names, pass_names;

	// hipEvent_t ring per run of a frame: a sync entry must keep naming the record of the frame it was made in (the alternate copy
	// of a double-buffered buffer was last read two frames ago), so the event of frame f is slot f % EventRing.  The
	// host never runs more than Device::StagingFrames - 1 frames ahead, so a slot is complete long before its reuse.
	enum { EventRing = 4 };
	static_assert(unsigned(EventRing) == HIP::Device::FrameFenceRing, "a run published under a device fence must stay named for as long as one under the graph's own events");
	std::vector<void *> pass_done_event;
	uint64_t frame_counter = 0;
	uint64_t last_device_frame = 0; // Device::get_frame_number() at the last enqueue (the two rings advance in lockstep)

	// the frame being enqueued
	HIP::Device *device = nullptr;
	size_t ring_slot = 0;
	uint64_t this_frame = 0, device_frame = 0, device_completed = 0;
	bool blit_follows = false;
	int expected_runs = 0;
	StreamType expected_stream = StreamType::Count;
	int last_run_of_stream[StreamCount] = {};
	// One event per RUN of consecutive passes on the same stream (not per pass): the accesses of every pass of the run are
	// published under the run's event, which is recorded once, after the run's last pass and before any pass of another
	// stream is enqueued.  Fewer packets between kernels: each event record / wait costs the command processor several
	// microseconds (measured: 23 us of a 283 us frame with one record per pass).
	StreamType run_stream = StreamType::Count; // stream of the run being enqueued
	unsigned run_slot = 0;                      // index of the run within the frame (event ring row)
	bool run_published = false;                 // a pass of the run published accesses under the run's event
	int current_pass = -1;
	std::vector<void *> waited; // by the current run

	void open_run(StreamType stream, unsigned slot);
	void close_run();
	void *run_event();
	void wait_for(const Access &access, const char *kind, unsigned resource);
};
} // namespace Granite
