#!/usr/bin/env python3
"""gtx_convert.py --format <name> --output out.gtx [--mipgen] in.gtx: compress an R8 / RG8 / RGBA8 .gtx on the GPU, after the
reference's tools/gtx_convert.cpp for the formats this build encodes.

    --format   bc4_unorm, bc5_unorm, or r8_unorm / rg8_unorm / rgba8_unorm (the input's own format: a copy)
    --mipgen   make the full mip chain from level 0 first; a chain the file has is made again
    --output   the .gtx to write

The reference tool's other options are not built here and are refused by name."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NOT_BUILT = {
    "--quality": "the RGTC compressor has one quality; the option belongs to the ISPC and astc-encoder formats, which are not built",
    "--swizzle": "swizzle_image is not built; the file's component swizzle is kept as it is",
    "--fixup-alpha": "fixup_alpha_edges is not built",
    "--alpha": "texture modes belong to the ISPC and astc-encoder formats, which are not built",
    "--deferred-mipgen": "the mipgen-on-load flag is not set by this tool; use --mipgen",
    "--normal-la": "texture modes belong to the ISPC and astc-encoder formats, which are not built",
    "--mask-la": "texture modes belong to the ISPC and astc-encoder formats, which are not built",
}
FORMATS = ("bc4_unorm", "bc5_unorm", "r8_unorm", "rg8_unorm", "rgba8_unorm")


class Refused(Exception):
    pass


def parse(argv):
    """(input path, output path, format name, mipgen) or Refused with the one-line reason."""
    for arg in argv:
        name = arg.split("=", 1)[0]
        if name in NOT_BUILT:
            raise Refused(f"{name} is not supported: {NOT_BUILT[name]}.")
    parser = argparse.ArgumentParser(prog="gtx_convert.py", add_help=True, allow_abbrev=False)
    parser.add_argument("--format", required=False)
    parser.add_argument("--output", required=False)
    parser.add_argument("--mipgen", action="store_true")
    parser.add_argument("input", nargs="?")
    try:
        args = parser.parse_args(argv)
    except SystemExit as e:
        if e.code == 0:
            raise
        raise Refused("Unknown or malformed option.") from None
    if not args.format:
        raise Refused("Must provide a format.")
    if args.format not in FORMATS:
        raise Refused(f"Unknown format: {args.format} (this build encodes {', '.join(FORMATS)}).")
    if not args.output or not args.input:
        raise Refused("Must provide input and output paths.")
    return args.input, args.output, args.format, args.mipgen


def main(argv):
    try:
        src, dst, fmt, mipgen = parse(argv)
    except Refused as e:
        print(e, file=sys.stderr)
        return 1
    from granite_amd import app as gapp
    application = gapp.Application(64, 64, lighting=False)
    try:
        application.encode_gtx(src, dst, fmt, mipgen=mipgen)
    except Exception as e:  # the library's reason, as one line
        print(f"Failed to convert {src}: {e}", file=sys.stderr)
        return 1
    finally:
        application.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
