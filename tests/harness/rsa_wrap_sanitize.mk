# The key wrap's arithmetic (jfsx_rsa.h) with its own main under
# AddressSanitizer and UBSan: a stand-alone host program, run where it is built
#   make -C tests/harness -f rsa_wrap_sanitize.mk run
# (tests/test_rsa_wrap.py::test_sanitized_standalone_run builds and runs the same).
# A makefile of its own, so that the harness Makefile stays as it is.
rsa_wrap_sanitize: rsa_wrap_host.cpp ../../juicefs_amd/csrc/jfsx_rsa.h
	g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
		-DRSA_WRAP_MAIN -o $@ rsa_wrap_host.cpp

run: rsa_wrap_sanitize
	./rsa_wrap_sanitize

clean:
	rm -f rsa_wrap_sanitize
.PHONY: run clean
