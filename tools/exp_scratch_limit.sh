D="${1:-build/scratch_limit}"; mkdir -p "$D"          # output directory (first argument)
for cfg in "X=1" "HSA_ENABLE_SCRATCH_ASYNC_RECLAIM=0" "HSA_SCRATCH_SINGLE_LIMIT_ASYNC=134217728" "HSA_SCRATCH_SINGLE_LIMIT=4294967296"; do
  tag=$(echo $cfg | tr '=' '_')
  env $cfg python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline > "$D/$tag.json" 2> "$D/$tag.err"
  echo "$cfg rc=$?"
  python - <<PY
import json
l=open("$D/$tag.json").read().strip().splitlines()[-1]
d=json.loads(l)
print({k:d.get(k) for k in ["ms_per_step","pairing_ms","mml_ms","equations_per_s","prepared_equations_per_s","prepared_equations_speedup"]}, d["extras"]["bls_verify_from_bytes"]["ms"])
PY
done
