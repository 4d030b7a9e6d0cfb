"""The one probe of include/kfac_hip.h's struct layouts that the ABI tests share: gcc compiles
a program that prints sizeof and offsetof, the tests compare with the ctypes mirrors."""
import os
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kfac_hip.h")


def c_layout(tmp_path, cname, fields=()):
    """[sizeof(cname)] + [offsetof(cname, f) for f in fields], as gcc lays the header's struct out."""
    src = tmp_path / f"{cname}.c"
    values = ", ".join([f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields])
    fmt = " ".join(["%zu"] * (1 + len(fields)))
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\n'
                   f'int main(void){{printf("{fmt}", {values}); return 0;}}\n')
    exe = tmp_path / cname
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return [int(v) for v in out.split()]
