// TEST INFRASTRUCTURE.  granite_amd/csrc/cacao_core.hpp -- the constant block, the workspace layout, the per-texel arithmetic and the kernel
// text that cacao.hip launches -- built for the host: the kernels run through tests/cpp/hip_emu.hpp with the launch geometry of
// cacao.hip, on a workspace in host memory.  tests/test_cacao_core_cpu.py builds it as a shared library (g++ -ffp-contract=off) and holds
// it to tests/cacao_ref.py before a device sees the code; with -DCACAO_HOST_MAIN it is a stand-alone program that runs the whole pass at
// two small odd sizes, which the same test builds with -fsanitize=address,undefined for the blur's LDS indexing and the guarded stores.
#include "hip_emu.hpp"
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#define CACAO_EMU 1
#include "../../granite_amd/csrc/cacao_core.hpp"
#include <cstdio>
#include <cstdlib>

using namespace gr_cacao;

static unsigned div_up(unsigned a, unsigned b) { return (a + b - 1) / b; }
static dim3 grid_for(uint32_t w, uint32_t h, uint32_t depth = 1) { return dim3(div_up(w, GROUP), div_up(h, GROUP), depth); }

extern "C" {
// offsets: depth_mip[4], normals, ssao[2], importance[2], load_counter, bytes
void cacao_host_layout(uint32_t width, uint32_t height, uint64_t offsets[11])
{
	const Workspace ws = workspace_layout(width, height);
	for (int k = 0; k < 4; k++)
		offsets[k] = ws.depth_mip[k];
	offsets[4] = ws.normals;
	offsets[5] = ws.ssao[0];
	offsets[6] = ws.ssao[1];
	offsets[7] = ws.importance[0];
	offsets[8] = ws.importance[1];
	offsets[9] = ws.load_counter;
	offsets[10] = ws.bytes;
}

float cacao_host_unorm8(uint32_t v) { return unorm8(v); }
void cacao_host_settings(gr_cacao_settings *s) { reference_settings(*s); }
void cacao_host_buffer_sizes(uint32_t width, uint32_t height, gr_cacao_buffer_sizes *b) { update_buffer_sizes(width, height, *b); }
void cacao_host_constants(gr_cacao_constants constants[4], const gr_cacao_settings *s, uint32_t width, uint32_t height, const float *proj, const float *view)
{
	gr_cacao_buffer_sizes b;
	update_buffer_sizes(width, height, b);
	for (int pass = 0; pass < 4; pass++)
	{
		constants[pass] = {};
		update_constants(constants[pass], *s, b, proj, view);
		update_per_pass_constants(constants[pass], b, pass);
	}
}

void cacao_host_prepare_depths(const void *depth, uint32_t width, uint32_t height, uint32_t pitch, void *workspace, const gr_cacao_constants *c)
{
	PrepareDepthsLaunch a = {};
	a.c = *c;
	a.depth = static_cast<const uint8_t *>(depth);
	a.depth_pitch = pitch;
	a.width = int(width);
	a.height = int(height);
	a.workspace = static_cast<uint8_t *>(workspace);
	a.ws = workspace_layout(width, height);
	emu::launch(k_cacao_prepare_depths, grid_for(a.ws.half_w, a.ws.half_h), dim3(GROUP, GROUP), a);
}

void cacao_host_prepare_normals(const void *normal, uint32_t width, uint32_t height, uint32_t pitch, void *workspace, const gr_cacao_constants *c)
{
	PrepareNormalsLaunch a = {};
	a.c = *c;
	a.normal = static_cast<const uint8_t *>(normal);
	a.normal_pitch = pitch;
	a.width = int(width);
	a.height = int(height);
	a.workspace = static_cast<uint8_t *>(workspace);
	a.ws = workspace_layout(width, height);
	emu::launch(k_cacao_prepare_normals, grid_for(a.ws.half_w, a.ws.half_h), dim3(GROUP, GROUP), a);
}

static GenerateLaunch generate_launch(void *workspace, const Workspace &ws, const gr_cacao_constants constants[4], uint32_t target)
{
	GenerateLaunch a = {};
	a.c = constants[0];
	a.pp = per_pass_of(constants);
	a.im = images_of(workspace, ws);
	for (uint32_t p = 0; p < PASSES; p++)
		a.out[p] = static_cast<uint8_t *>(workspace) + ws.ssao[target] + uint64_t(p) * ws.half_w * ws.half_h * 2u;
	return a;
}

// which: 0 = GenerateQ3Base (-> pong), 2 = GenerateQ2, 3 = GenerateQ3 (-> ping)
void cacao_host_generate(void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants constants[4], int which)
{
	const Workspace ws = workspace_layout(width, height);
	const GenerateLaunch a = generate_launch(workspace, ws, constants, which == 0 ? 1 : 0);
	const dim3 grid = grid_for(ws.half_w, ws.half_h, PASSES), block(GROUP, GROUP);
	if (which == 0)
		emu::launch(k_cacao_generate<3, true>, grid, block, a);
	else if (which == 2)
		emu::launch(k_cacao_generate<2, false>, grid, block, a);
	else
		emu::launch(k_cacao_generate<3, false>, grid, block, a);
}

// flags: 4 * half_h * half_w bytes, 1 where a tap's lod lies within 2^-10 of a mip switch
void cacao_host_generate_flags(const void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants constants[4], int which, uint8_t *flags)
{
	const Workspace ws = workspace_layout(width, height);
	const GenerateLaunch a = generate_launch(const_cast<void *>(workspace), ws, constants, 0);
	for (uint32_t p = 0; p < PASSES; p++)
		for (uint32_t y = 0; y < ws.half_h; y++)
			for (uint32_t x = 0; x < ws.half_w; x++)
			{
				float out[2];
				bool flag = false;
				if (which == 0)
					generate_texel<3, true>(a.c, a.pp, a.im, p, int(x), int(y), out, &flag);
				else if (which == 2)
					generate_texel<2, false>(a.c, a.pp, a.im, p, int(x), int(y), out, &flag);
				else
					generate_texel<3, false>(a.c, a.pp, a.im, p, int(x), int(y), out, &flag);
				flags[(size_t(p) * ws.half_h + y) * ws.half_w + x] = flag ? 1 : 0;
			}
}

// which: 0 = GenerateImportanceMap, 1 = PostprocessImportanceMapA, 2 = PostprocessImportanceMapB
void cacao_host_importance(void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *c, int which)
{
	const Workspace ws = workspace_layout(width, height);
	ImportanceLaunch a = {};
	a.c = *c;
	a.im = images_of(workspace, ws);
	uint8_t *base = static_cast<uint8_t *>(workspace);
	a.out = base + ws.importance[which == 1 ? 1 : 0];
	a.load_counter = reinterpret_cast<uint32_t *>(base + ws.load_counter);
	const dim3 grid = grid_for(ws.imp_w, ws.imp_h), block(GROUP, GROUP);
	// B: at most 3 workgroups here, so that even these small maps make a workgroup walk several groups, as the device's 2048 do at 4K
	const dim3 groups(grid.x * grid.y), walked(std::min(groups.x, 3u));
	if (which == 0)
		emu::launch(k_cacao_importance_generate, grid, block, a);
	else if (which == 1)
		emu::launch(k_cacao_importance_postprocess<false>, groups, block, a);
	else
		emu::launch(k_cacao_importance_postprocess<true>, walked, block, a);
}

void cacao_host_blur(void *workspace, uint32_t width, uint32_t height, const gr_cacao_constants *c, uint32_t blur_passes)
{
	const Workspace ws = workspace_layout(width, height);
	BlurLaunch a = {};
	a.c = *c;
	for (uint32_t p = 0; p < PASSES; p++)
	{
		a.in[p] = static_cast<const uint8_t *>(workspace) + ws.ssao[0] + uint64_t(p) * ws.half_w * ws.half_h * 2u;
		a.out[p] = static_cast<uint8_t *>(workspace) + ws.ssao[1] + uint64_t(p) * ws.half_w * ws.half_h * 2u;
	}
	a.half_w = int(ws.half_w);
	a.half_h = int(ws.half_h);
	a.blur_passes = blur_passes;
	const uint32_t tile_w = uint32_t(BLUR_TILE_W) * BLUR_GROUP - 2u * blur_passes, tile_h = uint32_t(BLUR_TILE_H) * BLUR_GROUP - 2u * blur_passes;
	emu::launch(k_cacao_blur, dim3(div_up(ws.half_w, tile_w), div_up(ws.half_h, tile_h), PASSES), dim3(BLUR_GROUP, BLUR_GROUP), a);
}

void cacao_host_apply(const void *workspace, void *out, uint32_t width, uint32_t height, uint32_t pitch, const gr_cacao_constants *c, uint32_t from_pong)
{
	const Workspace ws = workspace_layout(width, height);
	ApplyLaunch a = {};
	a.c = *c;
	a.im = images_of(workspace, ws);
	a.out = static_cast<uint8_t *>(out);
	a.out_pitch = pitch;
	a.width = int(width);
	a.height = int(height);
	a.from_pong = from_pong;
	emu::launch(k_cacao_apply, grid_for(width, height), dim3(GROUP, GROUP), a);
}
}

#if defined(CACAO_HOST_MAIN)
// The whole pass, HIGHEST with 2 and 8 blur passes and HIGH with 1, on exactly sized heap blocks: an access one byte past an image, the
// workspace or an LDS array is the sanitizers' to report.
static int run(uint32_t width, uint32_t height, uint32_t quality, uint32_t blur_passes)
{
	gr_cacao_settings s;
	reference_settings(s);
	s.quality_level = quality;
	s.blur_pass_count = blur_passes;
	const float proj[16] = {1.2990381f, 0, 0, 0, 0, -1.7320508f, 0, 0, 0, 0, 0.001001001f, -1, 0, 0, 0.1001001f, 0};
	const float view[16] = {1, 0, 0, 0, 0, 0.99227788f, 0.12403473f, 0, 0, -0.12403473f, 0.99227788f, 0, 0, -0.99227788f, -8.1862926f, 1};
	gr_cacao_constants c[4];
	cacao_host_constants(c, &s, width, height, proj, view);
	const Workspace ws = workspace_layout(width, height);
	uint8_t *workspace = static_cast<uint8_t *>(aligned_alloc(256, ws.bytes));
	float *depth = static_cast<float *>(malloc(size_t(width) * height * 4));
	uint32_t *normal = static_cast<uint32_t *>(malloc(size_t(width) * height * 4));
	uint8_t *out = static_cast<uint8_t *>(malloc(size_t(width) * height));
	memset(workspace, 0xcd, ws.bytes);
	uint32_t seed = 12345u;
	for (uint32_t y = 0; y < height; y++)
		for (uint32_t x = 0; x < width; x++)
		{
			seed = seed * 1664525u + 1013904223u;
			const float view_z = (x / 7 + y / 5) % 2 ? 3.0f + 0.01f * float(x) : 6.0f + float(seed >> 24) * 0.002f; // steps and slopes
			depth[y * width + x] = 0.1001001f / view_z - 0.001001001f;
			normal[y * width + x] = ((seed >> 8) & 1023u) | (((seed >> 3) & 1023u) << 10) | (800u << 20) | (3u << 30);
		}
	cacao_host_prepare_depths(depth, width, height, width * 4, workspace, &c[0]);
	cacao_host_prepare_normals(normal, width, height, width * 4, workspace, &c[0]);
	if (quality == GR_CACAO_QUALITY_HIGHEST)
	{
		cacao_host_generate(workspace, width, height, c, 0);
		for (int which = 0; which < 3; which++)
			cacao_host_importance(workspace, width, height, &c[0], which);
		cacao_host_generate(workspace, width, height, c, 3);
	}
	else
		cacao_host_generate(workspace, width, height, c, 2);
	if (blur_passes)
		cacao_host_blur(workspace, width, height, &c[0], blur_passes);
	cacao_host_apply(workspace, out, width, height, width, &c[0], blur_passes ? 1 : 0);
	uint32_t sum = 0;
	for (size_t i = 0; i < size_t(width) * height; i++)
		sum += out[i];
	printf("%ux%u quality %u blur %u: mean AO %.2f\n", width, height, quality, blur_passes, double(sum) / double(width * height));
	free(out);
	free(normal);
	free(depth);
	free(workspace);
	return 0;
}

int main()
{
	run(61, 45, GR_CACAO_QUALITY_HIGHEST, 2);
	run(16, 16, GR_CACAO_QUALITY_HIGHEST, 8);
	run(61, 45, GR_CACAO_QUALITY_HIGH, 1);
	run(130, 98, GR_CACAO_QUALITY_HIGH, 0);
	puts("cacao_core_host: done");
	return 0;
}
#endif
