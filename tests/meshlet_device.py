"""TEST SUPPORT.  One gr_meshlet_decode on the device with guard-filled outputs, returning the buffers in tests/meshlet_ref.decode's layout."""
import numpy as np

import meshlet_ref as mr
from granite_amd import capi


def device_decode(gr, streams, payload, offs, primitive_offset, vertex_offset, target, flags, caps, base_offset=0, wg_offsets=(0,), outputs=None):
    """caps: (primitives, vertices).  base_offset: bytes by which the index buffer's base pointer is moved inside its allocation.
    wg_offsets: one launch per entry, each with that wg_offset and so a grid shortened by it.  outputs: device buffers of an earlier call to
    decode into again.  Returns (dict of uint8 arrays, the device buffers); the index array is the bytes from the moved base on, and
    `before` the bytes in front of it."""
    nb = mr.index_bytes(flags)
    sizes = {"indices": caps[0] * 3 * nb + base_offset, "positions": caps[1] * 12, "attributes": caps[1] * 16, "skin": caps[1] * 8}
    meshlets, stream_count = streams.shape[:2]
    inputs = {"streams": np.ascontiguousarray(streams, np.uint32), "payload": np.ascontiguousarray(payload, np.uint32), "offsets": np.ascontiguousarray(offs, np.uint32)}
    dev_in = {k: capi.DeviceBuffer(gr, max(v.nbytes, 16)).upload(v) for k, v in inputs.items()}
    if outputs is None:
        outputs = {k: capi.DeviceBuffer(gr, max(n, 16)) for k, n in sizes.items()}
        for k, b in outputs.items():
            gr.check(gr.lib.gr_fill_byte(gr.handle, None, b.ptr, mr.GUARD, b.nbytes))
    a = capi.MeshletDecodeArgs()
    a.streams, a.payload, a.offsets = dev_in["streams"].ptr, dev_in["payload"].ptr, dev_in["offsets"].ptr
    a.payload_words, a.stream_count, a.target_style, a.flags = len(payload), stream_count, target, flags
    a.indices, a.positions, a.attributes, a.skin = outputs["indices"].ptr + base_offset, outputs["positions"].ptr, outputs["attributes"].ptr, outputs["skin"].ptr
    a.index_capacity, a.position_capacity, a.attribute_capacity, a.skin_capacity = caps[0], caps[1], caps[1], caps[1]
    for wg_offset in wg_offsets:
        gr.meshlet_decode(a, primitive_offset, vertex_offset, meshlets, wg_offset)
    gr.sync()
    got = {k: outputs[k].download(np.uint8, sizes[k]) for k in sizes}
    gr.sync()
    got["before"], got["indices"] = got["indices"][:base_offset], got["indices"][base_offset:]
    return got, outputs
