hipcc --offload-arch=gfx950 -O3 -o tools/gather_probe tools/gather_probe.hip
timeout -k 10 120 ./tools/gather_probe
