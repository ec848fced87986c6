#!/usr/bin/env python3
"""Bake an equirectangular environment on the GPU into the cubes deferred lighting's ENVIRONMENT path reads: the environment as a cube
with a full mip chain, its GGX-prefiltered reflection cube (128 texels a side, 8 levels) and its irradiance cube (32 texels a side).
The command line is that of the reference's tools/convert_equirect_to_environment.cpp."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--reflection", metavar="path.gtx", help="write the prefiltered reflection cube (128 x 128 x 6, 8 levels) here")
    p.add_argument("--irradiance", metavar="path.gtx", help="write the irradiance cube (32 x 32 x 6, 1 level) here")
    p.add_argument("--cube", metavar="path.gtx", help="write the environment cube (full mip chain) here")
    p.add_argument("--cube-scale", type=float, default=1.0, metavar="scale",
                   help="the cube is unsigned(scale * max(width / 3, height / 2)) texels a side (default 1)")
    p.add_argument("equirect", metavar="equirect.gtx",
                   help="the lat-long environment: a 2-D R16G16B16A16_SFLOAT .gtx.  Reading Radiance .hdr files is out of scope here: "
                        "convert them to .gtx first")
    return p


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    if not (args.reflection or args.irradiance or args.cube):
        print("nothing to do: none of --reflection, --irradiance, --cube was given", file=sys.stderr)
        return 1
    sys.path.insert(0, ROOT)
    from granite_amd import app as gapp
    application = gapp.Application(64, 64, lighting=False)
    try:
        application.bake_environment(args.equirect, cube=args.cube, reflection=args.reflection, irradiance=args.irradiance, cube_scale=args.cube_scale)
    finally:
        application.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
