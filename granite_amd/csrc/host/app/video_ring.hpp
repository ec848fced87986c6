// What frame recording and playback share: a non-blocking stream of their own and a ring of pinned host frames behind it.  A slot is
// filled by copies on the stream, its event recorded behind the last of them, and handed back in order; a full ring refuses a frame.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace Granite
{
struct VideoRing
{
	struct Slot
	{
		void *host[2] = {};        // pinned; recording uses the first alone
		hipEvent_t done = nullptr; // the frame's last copy on the stream is done
		int64_t frame = -1;
	};
	const char *who = "";      // "video recording" / "video playback": the prefix of what check() throws
	hipStream_t stream = nullptr;
	uint64_t bytes[2] = {};    // size of each of a slot's buffers; 0: none
	std::vector<Slot> slots;
	uint64_t written = 0, read = 0; // frames handed over / handed back

	void check(hipError_t err, const char *what) const
	{
		if (err != hipSuccess)
			throw std::runtime_error(std::string(who) + ": " + what + " failed: " + hipGetErrorString(err));
	}
	// the stream, then per slot its pinned buffers and its event; after a throw, release() undoes what was made
	void create(const char *who_, uint32_t frames, uint64_t bytes0, uint64_t bytes1 = 0)
	{
		who = who_;
		bytes[0] = bytes0;
		bytes[1] = bytes1;
		check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreateWithFlags");
		slots.resize(frames);
		for (auto &slot : slots)
		{
			for (int i = 0; i < 2; i++)
				if (bytes[i])
					check(hipHostMalloc(&slot.host[i], bytes[i], hipHostMallocDefault), "hipHostMalloc");
			check(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming), "hipEventCreateWithFlags");
		}
	}
	void release()
	{
		// frames may still be in flight: only this stream touches the slots
		if (stream)
			(void)hipStreamSynchronize(stream);
		for (auto &slot : slots)
		{
			for (void *host : slot.host)
				if (host)
					(void)hipHostFree(host);
			if (slot.done)
				(void)hipEventDestroy(slot.done);
		}
		slots.clear();
		if (stream)
			(void)hipStreamDestroy(stream);
		stream = nullptr;
	}
	void wait() const { check(hipStreamSynchronize(stream), "hipStreamSynchronize"); }
	bool full() const { return written - read >= slots.size(); }
	Slot &next_slot() { return slots[written % slots.size()]; }
	// records next_slot()'s event on the stream and numbers the frame: the slot is in use from here on
	void commit_slot()
	{
		Slot &slot = next_slot();
		check(hipEventRecord(slot.done, stream), "hipEventRecord");
		slot.frame = int64_t(written++);
	}
	// waits for the oldest unread frame's event (read != written), copies its buffer `which` to dst and hands the slot back
	void read_into(void *dst, unsigned which, int64_t *frame_number)
	{
		Slot &slot = slots[read % slots.size()];
		check(hipEventSynchronize(slot.done), "hipEventSynchronize");
		memcpy(dst, slot.host[which], bytes[which]);
		if (frame_number)
			*frame_number = slot.frame;
		read++;
	}
};
} // namespace Granite
