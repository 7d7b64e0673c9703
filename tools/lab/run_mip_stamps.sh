cd $GRAFT_REPO_ROOT
mkdir -p tools/_build gpurun_out
python -c "from xpoly_amd import build; build.build(extra=['-DXPG_STAMPS'], out='tools/_build/libxpoly_stamps.so', obj='tools/_build/obj_stamps')"
XPG_SO_PATH=$PWD/tools/_build/libxpoly_stamps.so PYTHONPATH=$PWD python tools/lab/probe_mip_stamps.py 2>&1 | tee gpurun_out/mip_stamps.log
