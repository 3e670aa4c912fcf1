#!/usr/bin/env python3
"""Per-kernel register / LDS / scratch use as hipcc reports it (-Rpass-analysis=kernel-resource-usage), one row per kernel.
usage: python tools/kernel_resources.py smelter_amd/csrc/smr_fused.hip [more .hip files] [-- extra hipcc flags]
       python tools/kernel_resources.py shader.co        a gfx950 code object (what smr_shader_program_code hands out: a user shader), or
       python tools/kernel_resources.py libsmr_hip.so    every code object of a built library — rows read from the AMDGPU metadata note"""
import os, re, struct, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smelter_amd import build as B

def demangle(n):
    try:
        return subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", n], capture_output=True, text=True).stdout.strip()
    except Exception:
        return n

def _msgpack(b, i=0):
    """The subset of MessagePack the AMDGPU metadata note uses -> (value, next offset)."""
    t = b[i]
    if t <= 0x7f: return t, i + 1
    if t >= 0xe0: return t - 256, i + 1
    if 0x80 <= t <= 0x8f or t in (0xde, 0xdf):
        n, i = (t & 15, i + 1) if t <= 0x8f else (struct.unpack_from(">H" if t == 0xde else ">I", b, i + 1)[0], i + (3 if t == 0xde else 5))
        out = {}
        for _ in range(n):
            k, i = _msgpack(b, i); v, i = _msgpack(b, i); out[k] = v
        return out, i
    if 0x90 <= t <= 0x9f or t in (0xdc, 0xdd):
        n, i = (t & 15, i + 1) if t <= 0x9f else (struct.unpack_from(">H" if t == 0xdc else ">I", b, i + 1)[0], i + (3 if t == 0xdc else 5))
        out = []
        for _ in range(n):
            v, i = _msgpack(b, i); out.append(v)
        return out, i
    if 0xa0 <= t <= 0xbf or t in (0xd9, 0xda, 0xdb, 0xc4, 0xc5, 0xc6):
        if t <= 0xbf: n, i = t & 31, i + 1
        else:
            w = {0xd9: 1, 0xda: 2, 0xdb: 4, 0xc4: 1, 0xc5: 2, 0xc6: 4}[t]
            n, i = int.from_bytes(b[i + 1:i + 1 + w], "big"), i + 1 + w
        raw = bytes(b[i:i + n])
        return (raw.decode(errors="replace") if t not in (0xc4, 0xc5, 0xc6) else raw), i + n
    if t == 0xc0: return None, i + 1
    if t in (0xc2, 0xc3): return t == 0xc3, i + 1
    fixed = {0xcc: ">B", 0xcd: ">H", 0xce: ">I", 0xcf: ">Q", 0xd0: ">b", 0xd1: ">h", 0xd2: ">i", 0xd3: ">q", 0xca: ">f", 0xcb: ">d"}
    if t in fixed:
        return struct.unpack_from(fixed[t], b, i + 1)[0], i + 1 + struct.calcsize(fixed[t])
    raise ValueError(f"msgpack type 0x{t:02x}")


def code_object_resources(elf: bytes) -> dict:
    """kernel name -> {vgpr, agpr, sgpr, scratch (bytes per lane), lds (bytes per workgroup), kernarg} from the NT_AMDGPU_METADATA note of
    a code object (an ELF64 image: smr_shader_program_code, or one bundle entry of a library's .hip_fatbin)."""
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        raise ValueError("not an ELF64 code object")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    out = {}
    for k in range(shnum):
        _name, stype, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + k * shentsize)
        if stype != 7:  # SHT_NOTE
            continue
        i, end = off, off + size
        while i + 12 <= end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, i)
            name_at = i + 12
            desc_at = name_at + ((namesz + 3) & ~3)
            if ntype == 32 and elf[name_at:name_at + 6] == b"AMDGPU":
                meta, _ = _msgpack(elf[desc_at:desc_at + descsz])
                for kern in meta.get("amdhsa.kernels", []):
                    out[kern[".name"]] = {"vgpr": kern.get(".vgpr_count"), "agpr": kern.get(".agpr_count", 0), "sgpr": kern.get(".sgpr_count"),
                                          "scratch": kern.get(".private_segment_fixed_size"), "lds": kern.get(".group_segment_fixed_size"),
                                          "kernarg": kern.get(".kernarg_segment_size")}
            i = desc_at + ((descsz + 3) & ~3)
    return out


def library_code_objects(lib: str = B.LIB) -> list:
    """The gfx code objects of a built library's .hip_fatbin section (the walk of smelter_amd.build.kernels_sha256)."""
    with open(lib, "rb") as f:
        data = f.read()
    off, size = B._elf_sections(data)[".hip_fatbin"]
    fb, magic, out, pos = data[off:off + size], b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (pos := fb.find(magic, pos)) >= 0:
        n, = struct.unpack_from("<Q", fb, pos + len(magic))
        p = pos + len(magic) + 8
        for _ in range(n):
            eoff, esize, tlen = struct.unpack_from("<QQQ", fb, p)
            p += 24
            if b"amdgcn" in fb[p:p + tlen] and esize:
                out.append(fb[pos + eoff:pos + eoff + esize])
            p += tlen
        pos += len(magic)
    return out


def library_resources(lib: str = B.LIB) -> dict:
    out = {}
    for elf in library_code_objects(lib):
        out.update(code_object_resources(elf))
    return out


def print_resources(title, res):
    print(f"# {title}")
    print(f"{'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'scr':>5} {'LDS':>7} {'karg':>5}  kernel")
    for name, r in res.items():
        nm = re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::", "", demangle(name) if name.startswith("_Z") else name))
        print(f"{r['vgpr']:>5} {r['agpr']:>5} {r['sgpr']:>5} {r['scratch']:>5} {r['lds']:>7} {r['kernarg']:>5}  {nm}")


def main():
    args = sys.argv[1:]
    extra = []
    if "--" in args:
        i = args.index("--"); extra = args[i + 1:]; args = args[:i]
    for src in args:
        with open(src, "rb") as f:
            head = f.read(4)
        if head == b"\x7fELF":  # a code object, or a built library
            with open(src, "rb") as f:
                data = f.read()
            print_resources(src, library_resources(src) if ".hip_fatbin" in B._elf_sections(data) else code_object_resources(data))
            continue
        cmd = [B.HIPCC] + B.FLAGS + extra + ["-x", "hip", "-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, capture_output=True, text=True).stderr
        rows, cur = [], None
        for line in err.splitlines():
            m = re.search(r"remark: [^:]*:\d+:\d+: (.*) \[-Rpass", line) or re.search(r"remark: (.*) \[-Rpass", line)
            if not m: continue
            t = m.group(1).strip()
            if t.startswith("Function Name:"):
                cur = {"name": demangle(t.split(":", 1)[1].strip())}; rows.append(cur)
            elif cur is not None and ":" in t:
                k, v = t.split(":", 1); cur[k.strip()] = v.strip()
        print(f"# {src}")
        print(f"{'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'scr':>5} {'occ':>4} {'LDS':>7}  kernel")
        for r in rows:
            nm = re.sub(r"\(anonymous namespace\)::", "", r["name"])
            nm = re.sub(r"\(.*$", "", nm)
            print(f"{r.get('VGPRs','?'):>5} {r.get('AGPRs','?'):>5} {r.get('TotalSGPRs', r.get('SGPRs','?')):>5} {r.get('ScratchSize [bytes/lane]','?'):>5} "
                  f"{r.get('Occupancy [waves/SIMD]','?'):>4} {r.get('LDS Size [bytes/block]','?'):>7}  {nm}")

if __name__ == "__main__":
    main()
