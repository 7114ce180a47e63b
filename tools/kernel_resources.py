"""The register / scratch / LDS budget and the machine-code hash of the kernels
in a built library (no GPU needed; it reads files only):

    python tools/kernel_resources.py [lib.so] [filter]
        one line per kernel whose symbol contains `filter` (default "render_"):
        VGPRs, SGPRs, scratch bytes, spilled VGPRs, static LDS bytes and the sha1
        of its gfx950 code.

    python tools/kernel_resources.py --diff old.so new.so [filter]
        the same lines for the kernels the two libraries share ("=": every figure
        and the hash are equal, "!": not), then the kernels only one of them
        holds ("-", "+") and the counts; exit status 1 unless all are equal.

The AMDGPU metadata is read as tests/test_kernel_resources.py reads it, the
code through a_dive_into_ray_tracing_amd/codeobj.py."""
import hashlib
import os
import pathlib
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_kernel_resources as K  # noqa: E402
from a_dive_into_ray_tracing_amd.codeobj import gfx950_code_objects, kernel_code  # noqa: E402


def kernel_table(lib, pat):
    """{kernel symbol: its metadata fields and "sha1"} of the library's gfx950 kernels whose symbol contains pat."""
    with tempfile.TemporaryDirectory() as d:
        meta = K.kernel_metadata(pathlib.Path(d), lib)
    with open(lib, "rb") as f:
        objects = gfx950_code_objects(f.read())
    table = {}
    for name, m in meta.items():
        sym = name[:-3] if name.endswith(".kd") else name  # (the metadata names the kernel descriptor)
        if pat not in sym:
            continue
        code = [r[1] for r in (kernel_code(co, sym) for co in objects) if r and r[0] == sym]
        table[sym] = dict(m, sha1=hashlib.sha1(code[0]).hexdigest() if code else None)
    return table


def line(name, m):
    return (f"{name:60s} vgpr {m.get('vgpr_count')} sgpr {m.get('sgpr_count')} scratch {m.get('private_segment_fixed_size')} "
            f"spill {m.get('vgpr_spill_count', 0)} lds {m.get('group_segment_fixed_size')} sha1 {m.get('sha1')}")


def diff(old, new, pat):
    """Prints the comparison; the number of kernels that differ or that only one library holds."""
    a, b = kernel_table(old, pat), kernel_table(new, pat)
    both = sorted(set(a) & set(b))
    changed = [k for k in both if a[k] != b[k]]
    print(f"# old: {len(a)} kernels matching '{pat}' in {old}")
    print(f"# new: {len(b)} kernels matching '{pat}' in {new}")
    for k in both:
        print(("! " if k in changed else "= ") + line(k, a[k]))
        if k in changed:
            print("  now " + line("", b[k]).strip())
    for k in sorted(set(a) - set(b)):
        print("- " + line(k, a[k]))
    for k in sorted(set(b) - set(a)):
        print("+ " + line(k, b[k]))
    print(f"# in both {len(both)}: equal {len(both) - len(changed)}, different {len(changed)}; "
          f"only old {len(set(a) - set(b))}, only new {len(set(b) - set(a))}")
    return len(changed) + len(set(a) ^ set(b))


def main(argv):
    if argv and argv[0] == "--diff":
        if len(argv) < 3:
            sys.exit(__doc__)
        return 1 if diff(argv[1], argv[2], argv[3] if len(argv) > 3 else "render_") else 0
    table = kernel_table(argv[0] if argv else K.LIB, argv[1] if len(argv) > 1 else "render_")
    for name in sorted(table):
        print(line(name, table[name]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
