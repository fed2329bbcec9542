"""`python prepro_dense.py ...` — the matched-paragraph file of the reference's qa/prepro_dense.py (process_ground_paras)."""
from proqa_amd.prepro_dense import main

if __name__ == "__main__":
    main()
