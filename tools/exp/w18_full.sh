cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
for l in ${LIBS:-libcompu_hip.so libcompu_hip_w18.so libcompu_hip_g320.so libcompu_hip.so libcompu_hip_w18.so}; do
  COMPU_HIP_LIB=$PWD/compu_amd/$l python bench.py --workload ${WL:-dynamic} --steps 10 --warmup 2 --no-cpu --extra 0 | python3 -c "import sys,json; b=json.loads(sys.stdin.read()); print('$l', b['roofline']['kernel_ms_avg'], b['verified_bit_exact'] if 'verified_bit_exact' in b else '')"
done
