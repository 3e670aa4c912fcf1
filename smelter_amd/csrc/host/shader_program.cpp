// shader_program.cpp — user shaders, host half: a fragment function written in HIP C++ becomes a gfx950 code object at registration
// time (include/smr.h "user shaders").  The ROCm runtime compiler (libhiprtc.so) is loaded with dlopen the first
// time a program is created — the library has no link dependency on it, and a host that never registers a shader source never loads
// it.  Needs no device and no context.  The program text is the library's own: smr_shader_dev.h (the texel helpers the built-in
// shaders are compiled from) and smr_user_shader_prelude.h around the user's translation unit, both embedded by smelter_amd/build.py.
#include "shader_program.h"

#include <dlfcn.h>

#include <cstring>
#include <mutex>

#include "smr_shader_prelude.inc"  // SMR_TEXT_SMR_SHADER_DEV_H, SMR_TEXT_SMR_USER_SHADER_PRELUDE_H (generated into the build directory)

// the user-shader launch of the device half (smr_user_shader.hip)
extern "C" int smr_user_shader(smr_ctx *ctx, const smr_shader_program *p, const void *params, size_t params_size, const smr_surface *const *src,
                               uint32_t n_src, smr_surface *dst, float time_s);

namespace {

// <hip/hiprtc.h>, the eight entry points this file uses (hiprtcResult: 0 = success)
struct Hiprtc {
    void *lib = nullptr;
    std::string why;
    const char *(*GetErrorString)(int) = nullptr;
    int (*CreateProgram)(void **prog, const char *src, const char *name, int n_headers, const char **headers, const char **include_names) = nullptr;
    int (*CompileProgram)(void *prog, int n_options, const char **options) = nullptr;
    int (*GetProgramLogSize)(void *prog, size_t *size) = nullptr;
    int (*GetProgramLog)(void *prog, char *log) = nullptr;
    int (*GetCodeSize)(void *prog, size_t *size) = nullptr;
    int (*GetCode)(void *prog, char *code) = nullptr;
    int (*DestroyProgram)(void **prog) = nullptr;
};

const Hiprtc *hiprtc() {
    static Hiprtc h;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6", "/opt/rocm/lib/libhiprtc.so"}) {
            h.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h.lib) break;
        }
        if (!h.lib) {
            const char *e = dlerror();  // (one call: dlerror() clears the message it returns)
            h.why = std::string("libhiprtc.so could not be loaded: ") + (e ? e : "?");
            return;
        }
        auto sym = [&](const char *n) {
            void *p = dlsym(h.lib, n);
            if (!p && h.why.empty()) h.why = std::string("libhiprtc.so lacks ") + n;
            return p;
        };
        h.GetErrorString = (decltype(h.GetErrorString))sym("hiprtcGetErrorString");
        h.CreateProgram = (decltype(h.CreateProgram))sym("hiprtcCreateProgram");
        h.CompileProgram = (decltype(h.CompileProgram))sym("hiprtcCompileProgram");
        h.GetProgramLogSize = (decltype(h.GetProgramLogSize))sym("hiprtcGetProgramLogSize");
        h.GetProgramLog = (decltype(h.GetProgramLog))sym("hiprtcGetProgramLog");
        h.GetCodeSize = (decltype(h.GetCodeSize))sym("hiprtcGetCodeSize");
        h.GetCode = (decltype(h.GetCode))sym("hiprtcGetCode");
        h.DestroyProgram = (decltype(h.DestroyProgram))sym("hiprtcDestroyProgram");
    });
    return &h;
}

// SMR_OK: p->code is the code object.  Otherwise p->log says why (the compiler's messages name the user's own lines: "shader:LINE:COL").
int compile(smr_shader_program *p, const char *source) {
    const Hiprtc *rtc = hiprtc();
    if (!rtc->why.empty()) {
        p->log = rtc->why;
        return SMR_ERR_INTERNAL;
    }
    std::string text = "#include \"smr_shader_dev.h\"\n#include \"smr_user_shader_prelude.h\"\n#line 1 \"shader\"\n";
    text += source;
    text += "\n#line 1 \"smr_user_shader_kernel\"\n#define SMR_USER_SHADER_KERNEL\n#include \"smr_user_shader_prelude.h\"\n";
    const char *headers[] = {SMR_TEXT_SMR_SHADER_DEV_H, SMR_TEXT_SMR_USER_SHADER_PRELUDE_H};
    const char *names[] = {"smr_shader_dev.h", "smr_user_shader_prelude.h"};
    void *prog = nullptr;
    int rc = rtc->CreateProgram(&prog, text.c_str(), "smr_user_shader", 2, headers, names);
    if (rc != 0) {
        p->log = std::string("hiprtcCreateProgram: ") + rtc->GetErrorString(rc);
        return SMR_ERR_INTERNAL;
    }
    // the library's own flags (smelter_amd/build.py FLAGS): a fragment restated from a built-in is rounded like the built-in
    const char *options[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"};
    rc = rtc->CompileProgram(prog, 4, options);
    size_t n = 0;
    if (rtc->GetProgramLogSize(prog, &n) == 0 && n > 1) {
        std::vector<char> log(n + 1, 0);
        if (rtc->GetProgramLog(prog, log.data()) == 0) p->log = log.data();
    }
    int out = SMR_OK;
    if (rc != 0) {
        if (p->log.empty()) p->log = std::string("hiprtcCompileProgram: ") + rtc->GetErrorString(rc);
        out = SMR_ERR_INVALID;
    } else if (rtc->GetCodeSize(prog, &n) != 0 || n < 4) {
        p->log += "hiprtcGetCodeSize: no code object";
        out = SMR_ERR_INTERNAL;
    } else {
        p->code.resize(n);
        if (rtc->GetCode(prog, p->code.data()) != 0 || memcmp(p->code.data(), "\x7f" "ELF", 4) != 0) {
            p->code.clear();
            p->log += "hiprtcGetCode: not an ELF code object";
            out = SMR_ERR_INTERNAL;
        }
    }
    rtc->DestroyProgram(&prog);
    p->ok = out == SMR_OK;
    return out;
}

int launch_program(void *user, smr_ctx *ctx, const void *params, size_t params_size, const smr_surface *const *src, uint32_t n_src,
                   smr_surface *dst, float time_s) {
    return smr_user_shader(ctx, (const smr_shader_program *)user, params, params_size, src, n_src, dst, time_s);
}
void release_program(void *user) { smr_shader_program_destroy((smr_shader_program *)user); }

}  // namespace

extern "C" {

SMR_API int smr_shader_program_create(const char *hip_source, smr_shader_program **out) {
    if (!out) return SMR_ERR_INVALID;
    *out = nullptr;
    if (!hip_source) return SMR_ERR_INVALID;
    smr_shader_program *p = new smr_shader_program();
    *out = p;  // also when the source does not compile: the log is the answer
    return compile(p, hip_source);
}

SMR_API const char *smr_shader_program_log(const smr_shader_program *p) { return p ? p->log.c_str() : "null program"; }

SMR_API int smr_shader_program_code(const smr_shader_program *p, const void **code, size_t *size) {
    if (!p || !code || !size || !p->ok) return SMR_ERR_INVALID;
    *code = p->code.data();
    *size = p->code.size();
    return SMR_OK;
}

SMR_API int smr_shader_program_launches(const smr_shader_program *p, uint64_t *count) {
    if (!p || !count) return SMR_ERR_INVALID;
    *count = p->launches.load(std::memory_order_relaxed);
    return SMR_OK;
}

SMR_API void smr_shader_program_destroy(smr_shader_program *p) {
    if (!p) return;
    if (p->unload) p->unload(p);
    delete p;
}

SMR_API int smr_renderer_register_shader_source(smr_renderer *r, const char *shader_id, const char *hip_source) {
    if (!r || !shader_id || !hip_source) return smr_renderer_fail(r, SMR_ERR_INVALID, "smr_renderer_register_shader_source: null argument");
    smr_shader_program *p = nullptr;
    const int rc = smr_shader_program_create(hip_source, &p);
    if (rc < 0) {  // RegisterRendererError: the registry keeps what it had
        const std::string log = p ? p->log : "out of memory";
        smr_shader_program_destroy(p);
        return smr_renderer_fail(r, rc, std::string("Failed to register shader \"") + shader_id + "\": " + log);
    }
    smr_shader_hook hook;
    hook.user = p;
    hook.launch = launch_program;
    hook.release = release_program;
    return smr_renderer_register_shader_hook(r, shader_id, hook);
}

SMR_API int smr_renderer_register_shader_program(smr_renderer *r, const char *shader_id, const smr_shader_program *p) {
    if (!r || !shader_id || !p) return smr_renderer_fail(r, SMR_ERR_INVALID, "smr_renderer_register_shader_program: null argument");
    if (!p->ok) return smr_renderer_fail(r, SMR_ERR_INVALID, std::string("Failed to register shader \"") + shader_id + "\": the program did not compile: " + p->log);
    smr_shader_hook hook;
    hook.user = (void *)p;
    hook.launch = launch_program;  // (not owned: no release)
    return smr_renderer_register_shader_hook(r, shader_id, hook);
}

}  // extern "C"
