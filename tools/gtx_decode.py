#!/usr/bin/env python3
"""gtx_decode.py src.gtx dst.gtx: decode a block-compressed (BC1-BC7 or ASTC LDR) .gtx on the GPU into an uncompressed one."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from granite_amd import app as gapp  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    application = gapp.Application(64, 64, lighting=False)
    application.decode_gtx(sys.argv[1], sys.argv[2])
    application.close()
