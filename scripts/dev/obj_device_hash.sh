#!/bin/bash
# developer tool: per object file of a build (obj_device_hash.sh <dir with *.o>), the sha256 of its gfx950 device code's disassembly (llvm-objdump -d
# --no-show-raw-insn, without the header lines that name the file) and of its kernel notes (registers, spills, scratch, LDS, kernarg size: llvm-readelf --notes).
# Two builds whose lines are equal run the same device code (the code objects themselves differ in a few bytes with the build directory).
L=/opt/rocm/lib/llvm/bin
for o in "$1"/*.o; do
    T=$(mktemp -d); cp "$o" $T/o.o
    (cd $T && $L/llvm-objdump --offloading o.o > /dev/null 2>&1)
    for f in $T/o.o.*gfx950; do
        d=$($L/llvm-objdump -d --no-show-raw-insn "$f" | grep -v "file format" | sha256sum | cut -c1-16)
        n=$($L/llvm-objdump -d --no-show-raw-insn "$f" | wc -l)
        k=$($L/llvm-readelf --notes "$f" | grep -vE "^(File|Displaying)" | sha256sum | cut -c1-16)
        echo "$(basename $o) disasm $d ($n lines) notes $k"
    done
    rm -rf $T
done
