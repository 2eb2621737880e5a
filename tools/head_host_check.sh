# AddressSanitizer + UBSan run of the prediction-head C-ABI's host code (workspace plan, argument validation) as a
# stand-alone program: tools/head_host_check.cpp linked with bcnf_amd/csrc/bcnf_head.hip, host side sanitized, device
# code untouched. No GPU needed, nothing preloaded:  bash tools/head_host_check.sh
set -e
cd "$(dirname "$0")/.."
mkdir -p build_exp
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -std=c++17 -Iinclude \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -g \
  bcnf_amd/csrc/bcnf_head.hip tools/head_host_check.cpp -o build_exp/head_host_check
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build_exp/head_host_check
