// TEST INFRASTRUCTURE.  The runner tests/golden/make_cacao_golden.py compiles next to the reference's own
// renderer/post/ffx-cacao/src/ffx_cacao.cpp (-I.../ffx-cacao/inc): it calls FFX_CACAO_UpdateBufferSizeInfo, FFX_CACAO_UpdateConstants and
// FFX_CACAO_UpdatePerPassConstants the way FFX_CACAO_GraniteDraw does (ffx_cacao_impl.cpp:776-781) and hands back the bytes.  Only those
// bytes are kept.
#include "ffx_cacao.h"
#include <string.h>

extern "C" unsigned cacao_runner_sizes(unsigned which) { return which == 0 ? sizeof(FFX_CACAO_Settings) : which == 1 ? sizeof(FFX_CACAO_Constants) : sizeof(FFX_CACAO_BufferSizeInfo); }

// settings: the 17 dwords of FFX_CACAO_Settings; proj, view: 16 floats each
extern "C" void cacao_runner_constants(unsigned width, unsigned height, const void *settings_words, const float *proj, const float *view,
                                       FFX_CACAO_BufferSizeInfo *bsi, FFX_CACAO_Constants constants[4])
{
	FFX_CACAO_Settings settings;
	memcpy(&settings, settings_words, sizeof(settings));
	FFX_CACAO_UpdateBufferSizeInfo(width, height, FFX_CACAO_FALSE, bsi);
	for (int i = 0; i < 4; i++)
	{
		memset(&constants[i], 0, sizeof(constants[i])); // the reference leaves Dummy0 as the stack had it
		FFX_CACAO_UpdateConstants(&constants[i], &settings, bsi, reinterpret_cast<const FFX_CACAO_Matrix4x4 *>(proj), reinterpret_cast<const FFX_CACAO_Matrix4x4 *>(view));
		FFX_CACAO_UpdatePerPassConstants(&constants[i], &settings, bsi, i);
	}
}
