// Follows MIT-licensed work (Granite, (c) 2017-2026 Hans-Kristian Arntzen; FidelityFX CACAO (c) 2016 Intel Corporation, modifications
// (c) 2021 Advanced Micro Devices, Inc.): see THIRD_PARTY_NOTICES.md at the repository root.
// renderer/post/ssao.{hpp,cpp} restated on the HIP executor: screen-space ambient occlusion by FidelityFX CACAO as Granite vendors it.
// Same pass and resource names, the same attachment declaration and the same settings; the dispatches of FFX_CACAO_GraniteDraw are the
// gr_cacao_* entry points (csrc/cacao.hip), all on the pass's stream.
#pragma once
#include <string>
#include "../render_context.hpp"
#include "../render_graph.hpp"

namespace Granite
{
// ssao.hpp:30-32.  Adds the compute pass `output` (ssao.cpp:45-122): storage texture `output`, R8_UNORM, the size of `input_depth`
// (D32_SFLOAT); texture inputs `input_depth` and `input_normal` (A2B10G10R10_UNORM_PACK32, the G-buffer's world-space normals).  The
// constants are made every frame from RenderParameters::projection and ::view; the workspace of intermediates is (re)made when the
// physical views change.  settings: null installs the reference's (ssao.cpp:73-91).  pass_name: empty names the pass like its output, as the
// reference does.  An empty input_normal asks for normals generated from depth, which this executor does not have: refused, like every
// setting gr_cacao_update_constants refuses.
void setup_ffx_cacao(RenderGraph &graph, const RenderContext &context, const std::string &output, const std::string &input_depth,
                     const std::string &input_normal, const gr_cacao_settings *settings = nullptr, const std::string &pass_name = {});
} // namespace Granite
