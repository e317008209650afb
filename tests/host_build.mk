# tests/host_build.mk — TEST-ONLY: the one recipe of the tests' host builds (g++, no GPU) of the product's device math.  A directory's
# Makefile sets what differs from the defaults and includes this file:
#   NAME         the library is _build/lib$(NAME).so (default: the directory's name)
#   SRC          its sources (default: every .cpp of the directory)
#   EXTRA        further compiler flags
#   FP_CONTRACT  the value of -ffp-contract (default: off)
#   PROGRAM      := 1 where the driver has a main behind #ifdef CBA_HOST_DRIVER_MAIN: adds _build/$(NAME)_san, the driver as a
#                stand-alone program under the address and undefined-behaviour sanitizers
# The library is the default goal, and the program is built only when it is named: nothing loaded into Python is sanitised.
# tests/host_build.py builds and loads either.
# -ffp-contract=off: the tests hold these builds to the bit against numpy restatements, which do not contract.  cpu_backend keeps gcc's
# default (fast): dense.hpp compiles chol_inplace_blocked for AVX2 with FMA, the one place where the flag changes the code.
# -Bsymbolic: a library shares inline (weak) symbols of the csrc headers with libcalibba.so; without it a process that has loaded both
# binds the library's calls to whichever copy was loaded first.
NAME ?= $(notdir $(CURDIR))
SRC ?= $(wildcard *.cpp)
CXX ?= g++
FP_CONTRACT ?= off
FLAGS := -std=c++17 -Wall -Wextra -Wno-unknown-pragmas -ffp-contract=$(FP_CONTRACT) $(EXTRA)
HDR := $(wildcard ../../calibration_amd/csrc/*.hpp) $(wildcard ../*.hpp) ../../include/calibba.h
_build/lib$(NAME).so: $(SRC) $(HDR)
	@mkdir -p _build
	$(CXX) -O2 $(FLAGS) -fPIC -shared -Wl,-Bsymbolic -o $@ $(SRC)
ifeq ($(PROGRAM),1)
_build/$(NAME)_san: $(SRC) $(HDR)
	@mkdir -p _build
	$(CXX) -O1 -g $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all -DCBA_HOST_DRIVER_MAIN -o $@ $(SRC)
endif
clean:
	rm -rf _build
.PHONY: clean
