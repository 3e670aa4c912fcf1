// smr_user_shader.hip — user shaders, device half: ShaderNode::render (transformations/shader/node.rs:71-89, shader/pipeline.rs:81-141)
// with the caller's own fragment function.  host/shader_program.cpp compiled the program (smr_user_shader_prelude.h around the user's
// text: k_shader_planes of smr_shaders.hip with its two switches replaced by calls); here its code object is loaded once per device and
// launched like smr_launch_plane_shader launches the built-ins — same grid, same stage, everything by value in the kernel arguments.
#include "smr_internal.h"

#include <algorithm>
#include <mutex>

#include "host/shader_program.h"

static_assert(SMR_USER_SHADER_SOURCES == SMR_SHADER_MAX_SOURCES && SMR_USER_SHADER_PARAM_BYTES == SMR_SHADER_MAX_PARAM_BYTES,
              "smr_shader_dev.h and include/smr.h disagree about a user shader's limits");
static_assert(sizeof(UserShaderArgs) + sizeof(void *) <= 4096, "kernel arguments: 4 KB at most");

namespace {

// programs that hold a module, for smr_user_shader_ctx_gone.  One lock for the list and for every program's module table: it is held
// for a table lookup per launch, and contexts are driven by one thread at a time (include/smr.h).
std::mutex g_live_mu;
std::vector<smr_shader_program *> g_live;

void unload_module(smr_shader_program::Module &m) {
    // (kernels of other streams of the device may still run the module's code: wait for the device, not for one stream)
    if (hipSetDevice(m.device) == hipSuccess) (void)hipDeviceSynchronize();
    if (m.module) (void)hipModuleUnload((hipModule_t)m.module);
    m.module = m.function = nullptr;
}

void unload_program(smr_shader_program *p) {
    std::lock_guard<std::mutex> g(g_live_mu);
    g_live.erase(std::remove(g_live.begin(), g_live.end(), p), g_live.end());
    for (auto &m : p->modules) unload_module(m);
    p->modules.clear();
}

}  // namespace

// smr_ctx_destroy: the modules this context was the last user of go with it
void smr_user_shader_ctx_gone(smr_ctx *ctx) {
    std::lock_guard<std::mutex> g(g_live_mu);
    for (smr_shader_program *p : g_live) {
        for (size_t i = 0; i < p->modules.size();) {
            auto &m = p->modules[i];
            m.users.erase(std::remove(m.users.begin(), m.users.end(), ctx), m.users.end());
            if (m.users.empty()) {
                unload_module(m);
                p->modules.erase(p->modules.begin() + (ptrdiff_t)i);
            } else {
                i++;
            }
        }
    }
}

extern "C" int smr_user_shader(smr_ctx *ctx, const smr_shader_program *program, const void *params, size_t params_size,
                               const smr_surface *const *src, uint32_t n_src, smr_surface *dst, float time_s) {
    SMR_ENTER(ctx);
    if (!ctx || !dst) return SMR_ERR_INVALID;
    smr_shader_program *p = const_cast<smr_shader_program *>(program);
    if (!p || !p->ok) return smr_fail(ctx, SMR_ERR_INVALID, "smr_user_shader: not a compiled program");
    if (dst->fmt != SMR_PX_RGBA8) return smr_fail(ctx, SMR_ERR_INVALID, "smr_user_shader: the target must be RGBA8");
    if (n_src > SMR_SHADER_MAX_SOURCES) return smr_fail(ctx, SMR_ERR_INVALID, "smr_user_shader: at most %d sources", SMR_SHADER_MAX_SOURCES);
    if (params_size > SMR_SHADER_MAX_PARAM_BYTES || (params_size && !params))
        return smr_fail(ctx, SMR_ERR_INVALID, "smr_user_shader: %zu parameter bytes (at most %d)", params_size, SMR_SHADER_MAX_PARAM_BYTES);
    UserShaderArgs a;
    memset(&a, 0, sizeof(a));
    a.dst = view_of(dst);
    a.n_src = (int)n_src;
    a.pxi = ctx->srgb() ? PXI_RGBA8_SRGB : PXI_RGBA8_UNORM;
    a.time = time_s;
    for (uint32_t i = 0; i < n_src; i++) {
        if (src && src[i]) {
            if (src[i]->fmt != SMR_PX_RGBA8) return smr_fail(ctx, SMR_ERR_INVALID, "smr_user_shader: source %u is not RGBA8", i);
            a.src[i] = view_of(src[i]);
        }
    }
    a.param_size = (u32)params_size;
    if (params_size) memcpy(a.params, params, params_size);

    hipFunction_t fn = nullptr;
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        smr_shader_program::Module *m = nullptr;
        for (auto &c : p->modules)
            if (c.device == ctx->device) m = &c;
        if (!m) {
            hipModule_t mod = nullptr;
            SMR_HIP(ctx, hipModuleLoadData(&mod, p->code.data()));
            hipError_t e = hipModuleGetFunction(&fn, mod, "smr_user_shader_kernel");
            if (e != hipSuccess) {
                (void)hipModuleUnload(mod);
                return smr_check_hip(ctx, e, "hipModuleGetFunction(smr_user_shader_kernel)");
            }
            smr_shader_program::Module nm;
            nm.device = ctx->device; nm.module = mod; nm.function = fn;
            p->modules.push_back(nm);
            m = &p->modules.back();
            if (!p->unload) {
                p->unload = unload_program;
                g_live.push_back(p);
            }
        }
        if (std::find(m->users.begin(), m->users.end(), ctx) == m->users.end()) m->users.push_back(ctx);
        fn = (hipFunction_t)m->function;
    }
    const float *tables = ctx->d_tables;
    void *args[] = {&a, &tables};
    StageScope scope(ctx, SMR_STAGE_LAYOUT);
    SMR_HIP(ctx, hipModuleLaunchKernel(fn, (dst->w + 63) / 64, (dst->h + 3) / 4, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
    p->launches.fetch_add(1, std::memory_order_relaxed);
    return SMR_OK;
}
