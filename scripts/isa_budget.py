"""Static issue budget of csrc/dsn_field16.hip: compiles the file to gfx950 assembly with build.py's own flags (no GPU needed) and
prints, per kernel,
  1. the instruction census: MFMA, other vector ALU (VALU), VALU per MFMA, accumulator-file moves (v_accvgpr_read_b32 /
     v_accvgpr_write_b32), packed f32 arithmetic (v_pk_*_f32), hazard / hand-written s_nop, LDS reads, LDS-DMA pieces,
  2. registers, scratch and spills from the code object's metadata,
  3. the per-gap histogram: how many other instructions are issued between one MFMA and the next (straight-line text order; a gap that
     crosses a branch or a label is counted with what the text holds), and a price of the MFMA stream by the one-wave-per-SIMD
     issue table: 8 cycles of issue for the MFMA itself, 4 per other instruction (8 for transcendentals), a gap lasting
     max(32, their sum).  The price is a model of issue slots, not a measurement: it knows nothing of waits.

    python scripts/isa_budget.py [--flags "<extra hipcc flags>"] [--kernels REGEX] [--src FILE] [--asm FILE.s]

Without --flags the file is compiled as build.py compiles it (its per-file flags included).  profiles/field16_isa_budget.txt holds
the output for the commit that introduced the script and for its parent."""
import argparse
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dual-space-nerf_amd")

SLOW = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32")
HIDDEN = 5                     # other instructions one 32x32x16 gap hides with one wave per SIMD


def build_module():
    spec = importlib.util.spec_from_file_location("dsn_build", os.path.join(PKG, "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def compile_asm(src, extra):
    b = build_module()
    flags = b.flags_for(src) + extra
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + flags + ["-S", "--offload-device-only", src, "-o", out], stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit("isa_budget.py: hipcc failed on %s with the flags above (exit status %d)" % (src, r.returncode))
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text, flags


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")
            return {n: re.sub(r"\(.*", "", re.sub(r"^void ", "", d)) for n, d in zip(names, out)}
        except Exception:
            continue
    return {n: n for n in names}


def kernels(text):
    """name -> list of instruction mnemonics (text order), name -> metadata dict"""
    body, meta = {}, {}
    lines = text.split("\n")
    starts = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            starts[m.group(1)] = i
        m = re.match(r"^\s+\.amdhsa_kernel (\S+)", ln)
        if m and m.group(1) in starts:
            ins = []
            for t in lines[starts[m.group(1)] + 1:i]:
                t = t.split(";")[0].strip()
                if not t or t.startswith(".") or t.endswith(":"):
                    continue
                ins.append(t.split()[0])
            body[m.group(1)] = ins
    name = None
    for ln in lines:
        m = re.match(r"^\s+\.name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
        m = re.match(r"^\s+\.(private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count|sgpr_count):\s+(\d+)", ln)
        if m and name in body:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
        m = re.match(r"^\s+\.set (\S+)\.num_(vgpr|agpr), (\d+)", ln)          # the two halves of the unified register file
        if m and m.group(1) in body:
            meta.setdefault(m.group(1), {})[m.group(2) + "_count"] = int(m.group(3))
    return body, meta


def census(ins):
    c = collections.Counter()
    for op in ins:
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op == "v_accvgpr_read_b32":
                c["acc_read"] += 1
            elif op == "v_accvgpr_write_b32":
                c["acc_write"] += 1
            elif op.startswith("v_pk_") and op.endswith("_f32"):
                c["pk_f32"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith("ds_read") or op.startswith("ds_load"):
            c["ds_read"] += 1
        elif op.startswith("global_load_lds"):
            c["lds_dma"] += 1
        elif op.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
    return c


def gaps(ins):
    """(histogram of other instructions per MFMA-to-MFMA gap, modelled cycles of the MFMA stream)"""
    hist, cycles = collections.Counter(), 0
    n, cost, seen = 0, 8, False
    for op in ins:
        if op.startswith("v_mfma"):
            if seen:
                hist[n] += 1
                cycles += max(32, cost)
            seen, n, cost = True, 0, 8
        elif seen and not op.startswith("s_branch") and not op.startswith("s_cbranch"):
            n += 1
            cost += 8 if op in SLOW else 4
    return hist, cycles


def report(text, want, out=sys.stdout):
    body, meta = kernels(text)
    names = [n for n in body if re.search(want, n)]
    pretty = demangle(names)
    p = lambda *a: print(*a, file=out)        # noqa: E731
    p("%-28s %6s %6s %9s %9s %9s %7s %6s %8s %8s" % ("kernel", "MFMA", "VALU", "VALU/MFMA", "acc_read", "acc_write", "pk_f32", "s_nop", "ds_read", "LDS-DMA"))
    for n in names:
        c = census(body[n])
        if not c["mfma"]:
            continue
        p("%-28s %6d %6d %9.2f %9d %9d %7d %6d %8d %8d" % (pretty[n][:28], c["mfma"], c["valu"], c["valu"] / c["mfma"], c["acc_read"],
                                                            c["acc_write"], c["pk_f32"], c["s_nop"], c["ds_read"], c["lds_dma"]))
    p()
    p("%-28s %6s %6s %6s %8s %12s %12s" % ("kernel", "VGPR", "AGPR", "SGPR", "scratch", "SGPR spills", "VGPR spills"))
    for n in names:
        m = meta.get(n, {})
        p("%-28s %6s %6s %6s %8s %12s %12s" % (pretty[n][:28], m.get("vgpr_count", "?"), m.get("agpr_count", "?"), m.get("sgpr_count", "?"),
                                             m.get("private_segment_fixed_size", "?"), m.get("sgpr_spill_count", "?"), m.get("vgpr_spill_count", "?")))
    p()
    p("other instructions per MFMA gap (%d hide; a gap lasts max(32, 8 + 4 per instruction) cycles in the model)" % HIDDEN)
    p("%-28s %s %7s %7s %9s %10s" % ("kernel", " ".join("%5s" % (str(k) if k < 12 else "12+") for k in range(13)), "<=1", ">%d" % HIDDEN, "cycles", "cyc/MFMA"))
    for n in names:
        h, cyc = gaps(body[n])
        tot = sum(h.values())
        if not tot:
            continue
        row = [h[k] for k in range(12)] + [sum(v for k, v in h.items() if k >= 12)]
        p("%-28s %s %7d %7d %9d %10.1f" % (pretty[n][:28], " ".join("%5d" % v for v in row), h[0] + h[1], sum(v for k, v in h.items() if k > HIDDEN),
                                          cyc, cyc / tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags", default="", help="extra hipcc flags (e.g. \"-DF16_SGB_VALU=3\")")
    ap.add_argument("--kernels", default="k_field16|k_light16|k_screen16|k_tangent16|k_adjoint16", help="regex on the mangled kernel name")
    ap.add_argument("--src", default=os.path.join(PKG, "csrc", "dsn_field16.hip"))
    ap.add_argument("--asm", default=None, help="an assembly listing made elsewhere instead of compiling")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            text = f.read()
        print("listing:", os.path.basename(a.asm))
    else:
        text, flags = compile_asm(a.src, a.flags.split())
        print("hipcc", " ".join(flags), "-S --offload-device-only", os.path.relpath(a.src, ROOT))
    report(text, a.kernels)


if __name__ == "__main__":
    main()
