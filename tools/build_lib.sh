# Plain (shipped-flags) build of the library under another name, for same-box A/B runs: bash tools/build_lib.sh head
set -e
cd "$(dirname "$0")/.."
mkdir -p build_exp
name=${1:-head}
shift || true
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Iinclude "$@" \
  bcnf_amd/csrc/bcnf_*.hip -o build_exp/lib$name.so    # every unit: the bindings take every entry point of the header
